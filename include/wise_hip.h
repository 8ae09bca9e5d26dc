/*
 * wise_hip.h — C ABI of libwise_hip.so: the MI355X (gfx950) hot paths of WISE.
 *
 * The reference (ox-vgg/wise) has no FFI of its own: its hot paths disappear into three Python
 * packages (open_clip, msclap, faiss).  Each entry point below replaces ONE such call and names the
 * reference call site it stands behind.  Everything is plain pointers + sizes: device pointers are
 * raw HBM addresses (any allocator: hipMalloc, torch), `stream` is a hipStream_t passed as void*.
 * No call allocates, frees or synchronises; all scratch comes from the caller's workspace, so every
 * entry point is hipGraph-capturable.
 *
 * Return value: 0 on success, otherwise a WISE_E_* code (<0) or a hipError_t (>0).
 * wise_last_error() returns a thread-local human-readable message for the last failure.
 */
#ifndef WISE_HIP_H
#define WISE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WISE_OK 0
#define WISE_E_INVALID (-1)   /* bad argument (shape, alignment, null pointer)          */
#define WISE_E_WORKSPACE (-2) /* workspace smaller than *_workspace_bytes() asks for    */
#define WISE_E_UNSUPPORTED (-3)

const char* wise_last_error(void);
/* ABI version of this header; bumped on any signature change (2: per-index counters for the two-stage search,
 * the shadow's error norm, wise_build_flags; 3: wise_vit_config.arch, wise_text_config.no_causal / eps_e6 — the SigLIP
 * towers — and the wise_xlmr_* entry points; 4: wise_xlmr_config.pos_mode / pool / head / eps_e12 — MS-CLAP 2022's BERT
 * caption encoder — and the wise_cnn14_* entry points; 5: wise_ip_shadow_i8 / wise_ip_topk_shadow8_f32 (int8 shadow,
 * norms[4]), wise_ip_topk_shadow_workspace_bytes depends on nq and returns 0 under 2^18 rows, two-stage k up to 1024; and,
 * added within 5: wise_vit_config.ln_fold, the wise_gemm_fold_* entry points, wise_attention_oproj_fold, wise_htsat_forward2,
 * wise_mlp_stream, wise_mlp_stream_ln, wise_swin_qkv_attn, the wise_ivf_* build entry points, wise_ivf_scan_local_*, the wise_pq_* entry points,
 * wise_ivfpq_scan, wise_ivf_refine and wise_ivf_refine_rows); also added within 5: wise_ivfpq_scan_local and
 * wise_ivf_refine_local, the last two stages on one rank's slice of an index sharded across GPUs; and wise_opq_rotate,
 * wise_opq_corr (with wise_opq_corr_workspace_bytes) and wise_opq_decode, the learned rotation of IndexIVFOPQ<m>; and
 * wise_sel_bitmap, wise_sel_positions (with wise_sel_positions_workspace_bytes), wise_ip_topk_pos_f32, wise_ivf_scan_sel_f32 and
 * wise_ivfpq_scan_sel, the searches restricted to a set of ids; and the wise_sq_* entry points with wise_ivfsq_scan,
 * wise_ivfsq_scan_sel and wise_ivfsq_scan_local, IndexIVFSQ8 and one rank's slice of it; and the count / fill pairs of
 * range_search, wise_ip_range_*, wise_ivf_range_* and wise_ivfsq_range_*; and wise_compact_plan (with wise_compact_plan_entries),
 * wise_compact_rank and wise_compact_rows, the in-place compaction behind remove_ids; and wise_sq16_encode, wise_sq16_decode,
 * wise_ivfsq16_scan (with _sel and _local) and wise_ivfsq16_range_count / _fill, IndexIVFSQfp16; and the wise_ipsq16_* entry points
 * (wise_ipsq16_topk, _topk_pos, _range_count / _fill, _reconstruct, _prepare, _topk_batched and the wise_ipsqfp16_*_workspace_bytes),
 * IndexSQfp16; and the wise_l2_* entry points (wise_l2_topk_f32, wise_l2_topk_pos_f32, wise_l2_range_count_f32 / _fill_f32,
 * wise_l2_prepare, wise_l2_topk_batched and their three workspace functions), IndexFlatL2; and wise_sq_minmax and the wise_ipsq8_*
 * entry points (wise_ipsq8_topk, _topk_pos, _range_count / _fill, _reconstruct, _prepare, _topk_batched and their three workspace
 * functions), IndexSQ8bit; and the wise_ivfl2_* entry points (wise_ivfl2_scan, _scan_sel, _scan_local, _range_count / _fill and their
 * three workspace functions) with wise_l2_half_norms, wise_ivf_l2_coarse and wise_ivf_list_means, IndexIVFFlatL2; and wise_pqflat_topk, wise_pqflat_topk_pos (with
 * wise_pqflat_topk_workspace_bytes) and wise_pqflat_decode, IndexPQ<m>; and the wise_l2sq16_* entry points (wise_l2sq16_topk, _topk_pos,
 * _range_count / _fill, _prepare, _topk_batched and their three workspace functions), IndexSQfp16L2; and the nine *_group_scores
 * entry points with wise_group_best, wise_group_topk and wise_group_workspace_bytes, search_grouped; and wise_sel_bitmap_groups
 * (with wise_sel_groups_workspace_bytes), wise_sel_bitmap_idbits and wise_sel_combine, the group selector, faiss's IDSelectorBitmap
 * and the And / Or / XOr / Not trees of selectors.  The version is 5. */
int wise_abi_version(void);
/* Host-side hint for the GEMM tile heuristic (no device work), local to the CALLING THREAD: on != 0 while this thread
 * enqueues batches that will run beside another stream's (two batches in flight); tilings that measured slower there
 * are then avoided for the shapes the one-wave-per-SIMD kernels do not take.  wise_vit_forward sets it itself for its
 * half batches; the engines' forward_pipelined bracket their calls with it.  Results never depend on it. */
void wise_overlap_hint(int on);
/* The compiler flags the device code of this library was built with (wise_amd/build.py).  The product kernels must
 * be built without packed f32 VALU math ("-fno-slp-vectorize ... -packed-fp32-ops": DESIGN.md section 4, a gfx950
 * wait-state hazard); __graft_entry__.smoke() and the tests assert it on the library that is actually loaded. */
const char* wise_build_flags(void);
/* 1 when a HIP device of arch gfx950 is visible to the calling process, else 0. */
int wise_device_ok(void);

/* Measurement aid (bench.py): between wise_prof_begin and wise_prof_end every bf16 GEMM launch
 * (class 0, work = flop) and every IP-scan launch (class 1, work = algorithmic bytes N*d*4) is
 * bracketed by a HIP event pair recorded on the launch stream.  wise_prof_end synchronises and
 * fills three arrays of length 2: summed milliseconds, launch counts, summed work.  Not thread-safe. */
int wise_prof_begin(int capacity);
int wise_prof_end(double* ms_sum, int64_t* launches, double* work_sum);

/* ------------------------------------------------------------------------------------------------
 * HP-2  brute-force inner-product top-k  (replaces faiss IndexIDMap{IndexFlatIP}::search,
 *       reference call sites src/index/feature_search_index.py:113 and api/routes.py:1407)
 *
 * X   [N,d]  fp32 row-major database rows resident in HBM (what faiss stores: :47-52,:81)
 * Q   [nq,d] fp32 queries (device)
 * ids [N]    int64 external ids (IndexIDMap, :52,:81) or NULL => id = id_base + row
 * outD [nq,k] fp32 descending; outI [nq,k] int64; tail padded with (-3.4028235e38, -1) when N < k
 *            (faiss semantics relied on by search.py:142-143, routes.py:1411)
 * Ties: the row with the lower position wins (faiss leaves tie order unspecified).
 * Limits: d % 4 == 0, 4 <= d <= 2048, 1 <= k <= 2048, 1 <= nq <= 1024, X 16-byte aligned.
 * Batches: nq < 8 (or k > 16, d > 512, d % 32 != 0) runs the single-pass VALU scan per group of up to 4
 * queries; nq >= 8 runs passes of 32 (or 64) queries on the matrix cores, one pass over X per pass: for k <= 12
 * candidates are ranked by split-bf16 products (error <= 2^-16 sum|x_c q_c|) and the best 16 per query are
 * re-scored in fp32, for 12 < k <= 16 the products themselves are fp32.
 * Every returned score is an fp32 dot product (different summation orders between paths: scores agree to ~1e-6
 * relative, ids agree wherever neighbouring scores differ by more than that).
 * ---------------------------------------------------------------------------------------------- */
size_t wise_ip_topk_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_ip_topk_f32(const float* X, int64_t N, int d, const float* Q, int nq, int k,
                     const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same search in two stages over a bf16 shadow copy of the rows (half the bytes of X per query), exact by
 * construction; first of all for ONE query, the reference's call shape (feature_search_index.py:113):
 *   wise_ip_shadow_bf16   Xb [N,d] bf16 (round-to-nearest-even copy of X) and two device floats norms[0] = max_r |X[r,:]|,
 *       norms[1] = max_r |X[r,:] - Xb[r,:]| (the largest rounding residual: a score computed from Xb differs from the
 *       exact one by at most eps = |q| norms[1] + f32 accumulation slack — Cauchy-Schwarz, no assumption on the data).
 *   wise_ip_topk_shadow_f32, one query (N >= 2^18; smaller indexes are answered by wise_ip_topk_f32 itself):
 *       (1) a sample of 64K rows (128 evenly spaced chunks) of Xb gives s_A, the k-th best approximate score seen;
 *           the exact k-th best score of the index is then >= s_A - eps, and a row of the exact top-k scores
 *           >= s_A - 2 eps approximately; (2) one pass over Xb collects EVERY row with approximate score >= s_A - 2 eps
 *           (typically 1-3 thousand of 10M; up to 262144); (3) the collected scores themselves give a sharper bound
 *           (their k-th largest slice maximum L: keep what reaches L - 2 eps, up to 16384 rows); (4) the scores of what
 *           is left are recomputed from the fp32 rows and the k best are written.  Nothing is certified after the fact
 *           and nothing depends on how the data is distributed (runs of near-duplicates — consecutive video frames —
 *           only make the lists longer).  (5) If a list overflows, the fp32 scan queued behind answers instead (it
 *           returns at once otherwise).
 *       All on the stream, no host round trip.
 * Any k <= 1024 for one query (the k WISE sends: REST `end` = 20, api/routes.py:1171,1407; evaluation k = 100 and
 * --topk 1000, docs/Search-Index-Evaluation.md:109, docs/Retrieval-Evaluation.md:39): the selections are radix selections,
 * and for k > 64 the collect pass runs in two ranges with the threshold tightened in between.
 * Two or more queries (k <= 12, d = 256 or 512; three or more with k <= 128 for d = 256 ... 1024, the fp32 VALU scan as the
 * gated fallback) run 128 / 64 / 32 queries at a time on the matrix cores in the same threshold form: the bf16 rows are MFMA
 * operands as loaded, every (query, row) that could matter is collected, re-scored in fp32 and the k best selected per
 * query; if any query's list overflows, the scan of the fp32 rows queued behind and gated redoes the pass.  Otherwise: one
 * query at a time.
 * counters (device, two int32, may be NULL): [0] += queries answered from the shadow, [1] += queries handed to the fp32
 * scan.  They belong to the caller (one pair per index); the library keeps no process-wide state for this.
 * Same outputs, ties and padding as wise_ip_topk_f32.  Limits: d % 8 == 0, 8 <= d <= 1024, k <= 1024, N >= 1, nq <= 1024. */
int wise_ip_shadow_bf16(const float* X, int64_t N, int d, uint16_t* Xb, float* norms /*[2]*/, void* stream);
size_t wise_ip_topk_shadow_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_ip_topk_shadow_f32(const float* X, const uint16_t* Xb, const float* norms /*[2]*/, int64_t N, int d, const float* Q,
                            int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                            int32_t* counters, void* workspace, size_t workspace_bytes, void* stream);

/* The same two-stage search over an INT8 shadow: a quarter of the bytes of X per query (N (d + 4) instead of 4 N d).
 *   wise_ip_shadow_i8   Xq [N,d] int8 = round(X[r,:] / scales[r]), scales[r] = max|X[r,:]| / 127, and four device floats:
 *       norms[0] = max_r |scales[r] Xq[r,:]|, norms[1] = the score error bound per unit |q| (the largest quantisation
 *       residual max_r |X[r,:] - scales[r] Xq[r,:]|, in norms[2], plus sqrt(d) 1.6e-5 norms[0] for the query, which the
 *       scans take as two int8 pieces); no assumption on the data: Cauchy-Schwarz, as for the bf16 shadow.
 *   wise_ip_topk_shadow8_f32   one query at a time in the threshold form of wise_ip_topk_shadow_f32 — sample, threshold,
 *       collect, refine, exact re-scoring from the fp32 rows, gated fp32 scan — with the two scans on v_dot4_i32_i8
 *       (integer sums: exact).  The bound is ~4x the bf16 shadow's, so a few hundred rows are re-scored instead of a
 *       few dozen; the results are the same bits as wise_ip_topk_f32's.  Workspace: wise_ip_topk_shadow_workspace_bytes.
 * Limits: d % 16 == 0, 16 <= d <= 1024, k <= 1024, nq <= 1024 (answered one by one). */
int wise_ip_shadow_i8(const float* X, int64_t N, int d, int8_t* Xq, float* scales /*[N]*/, float* norms /*[4]*/, void* stream);
int wise_ip_topk_shadow8_f32(const float* X, const int8_t* Xq, const float* scales, const float* norms /*[4]*/, int64_t N, int d,
                             const float* Q, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                             int32_t* counters, void* workspace, size_t workspace_bytes, void* stream);

/* IndexIVFFlat search, second stage (the first stage — the `nprobe` nearest centroids of each query — is
 * wise_ip_topk_f32 over the centroid table): scan the probed inverted lists and keep the k best.
 * Replaces faiss IndexIVFFlat::search as reached through self.index.search at
 * src/index/feature_search_index.py:113 for indexes built at :53-76 (nprobe set at api/routes.py:899-902).
 *   X        [N,d] fp32 rows grouped by list (list l occupies rows list_off[l] .. list_off[l+1]-1)
 *   list_off [nlist+1] int64;  ids [N] int64 external ids in the same order (NULL => the row number)
 *   probes   [nq,nprobe] int64 list numbers per query, entries < 0 are skipped
 * outD/outI as wise_ip_topk_f32 (descending scores, (-3.4028235e38, -1) padding).
 * Ties: the row that comes first in X wins. */
size_t wise_ivf_scan_workspace_bytes(int nq, int nprobe, int k);
int wise_ivf_scan_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                      const float* Q, int nq, const int64_t* probes, int nprobe, int k, float* outD, int64_t* outI,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same second stage on ONE RANK's slice of a list-major IndexIVFFlat sharded across GPUs (rank r holds rows
 * shard_range(N_total, r, W) of the lists laid end to end; wise_amd/index/sharded.py):
 *   X, ids   [N,d] / [N] this rank's rows (ids are the global external ids)
 *   list_off [nlist+1] the global offsets clipped to the slice (lists outside it are empty)
 *   probes   [nq,nprobe] GLOBAL list numbers (the coarse stage is replicated on every rank)
 * Probes whose local segment is empty are dropped on the device first (kept in probe order), so the scan and the merge
 * only work on the ~nprobe/W lists the rank holds.  probe_count [nq] (optional) receives the number kept per query.
 * outD/outI as wise_ivf_scan_f32 over the slice; wise_topk_merge of the ranks' answers in rank order then gives the same
 * bits as wise_ivf_scan_f32 over the whole array, ties included.  Limits: d % 4 == 0, d <= 2048, k <= 2048,
 * nprobe <= 2048.  Workspace: wise_ivf_scan_local_workspace_bytes(nq, nprobe, k) bytes. */
size_t wise_ivf_scan_local_workspace_bytes(int nq, int nprobe, int k);
int wise_ivf_scan_local_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                            const float* Q, int nq, const int64_t* probes, int nprobe, int k, float* outD, int64_t* outI,
                            int32_t* probe_count, void* workspace, size_t workspace_bytes, void* stream);

/* Dense scores [nq, N] = Q x X^T in exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain per
 * score).  The coarse stage of IndexIVFFlat when nprobe is a sizeable part of nlist — the reference's nprobe = 1024
 * (config.py:19, api/routes.py:899-902) over 10 round(sqrt(N)) cells: all centroid scores, then wise_select_topk_f32.
 * X [N,d], Q [nq,d] fp32, 16-byte aligned, d % 4 == 0. */
int wise_ip_scores_f32(const float* X, int64_t N, int d, const float* Q, int nq, float* scores, void* stream);
/* Indices of the k largest entries of each row of scores [rows, n] fp32 (ties: lower index), written in ascending
 * index order, -1 padding when n < k.  The second half of the coarse stage (scores from wise_ip_scores_f32).  NaN
 * scores are not supported. */
int wise_select_topk_f32(const float* scores, int rows, int n, int k, int64_t* out, void* stream);
/* (ABI 5) Building an IndexIVFFlat on the device without a vendor kernel: the bookkeeping of `index.train(features)` (spherical
 * k-means) and of `index.add_with_ids(...)` / the grouping by list (src/index/feature_search_index.py:53-76; faiss Clustering,
 * IndexIVF.add).  All deterministic: the same inputs give the same bits run after run.
 *   wise_ivf_argmax: out[r] = argmax_c scores[r, c] (ties: the lowest c; a row of NaNs: 0).
 *   wise_ivf_group: order [n] = the row numbers grouped by list, STABLE (rows of a list in ascending row number), list_off
 *     [nlist + 1] their offsets, counts [nlist] (or null); assign values in [0, nlist), nlist <= 2^24; workspace of
 *     wise_ivf_group_workspace_bytes(n, nlist) bytes.
 *   wise_ivf_list_sums: sums[c, :] = the sum of x[order[i], :] over list c's entries, added in that order (d % 4 == 0).
 *   wise_ivf_normalize_rows: out[r, :] = in[r, :] / max(||in[r, :]||, 1e-20) (may be in place).
 *   wise_ivf_reseed: sums[empty[e], :] = sums[donor[e], :] * (1 + 1e-3 sign(.)).
 *   wise_ivf_gather_rows / _i64: out[i] = x[idx[i]] (rows of d floats, d % 4 == 0 / int64 scalars).
 *   wise_ivf_expand_lists: out[list_off[c] .. list_off[c + 1]) = c. */
int wise_ivf_argmax(const float* scores, int rows, int n, int64_t* out, void* stream);
size_t wise_ivf_group_workspace_bytes(int64_t n, int nlist);
int wise_ivf_group(const int64_t* assign, int64_t n, int nlist, int64_t* order, int64_t* list_off, int64_t* counts, void* workspace,
                   size_t workspace_bytes, void* stream);
int wise_ivf_list_sums(const float* x, const int64_t* order, const int64_t* list_off, int nlist, int d, float* sums, void* stream);
int wise_ivf_normalize_rows(const float* in, int rows, int d, float* out, void* stream);
int wise_ivf_reseed(float* sums, const int64_t* empty, const int64_t* donor, int n_empty, int d, void* stream);
int wise_ivf_gather_rows(const float* x, const int64_t* idx, int64_t n, int d, float* out, void* stream);
int wise_ivf_gather_i64(const int64_t* a, const int64_t* idx, int64_t n, int64_t* out, void* stream);
int wise_ivf_expand_lists(const int64_t* list_off, int nlist, int64_t* out, void* stream);
/* (ABI 5, additive) IndexIVFPQ: inverted lists of 8-bit product-quantizer codes — faiss.IndexIVFPQ(IndexFlatIP(d), d, nlist, m, 8,
 * METRIC_INNER_PRODUCT) with by_residual (the index family of docs/Search-Index-Evaluation.md:105-123).  A row x of list l is kept as
 * m bytes: its residual x - c_l cut into m sub-vectors of dsub = d / m floats, each replaced by the number of its nearest (L2)
 * codeword.  codebooks [m, 256, dsub] fp32 are shared by all lists.  Limits (WISE_E_UNSUPPORTED otherwise): d % m == 0, m <= 128,
 * dsub even in [2, 96]; the scan: k <= 2048, nprobe <= 2048, nq <= 65535.  All deterministic: the same inputs give the same bits.
 *   wise_pq_residuals: out[i, :] = x[i, :] - centroids[assign[i], :] (assign values in [0, nlist)).
 *   wise_pq_encode: codes[i, j] = argmax_c (r_ij . cb_jc - 1/2 ||cb_jc||^2), both products index-ordered fmaf chains from 0, ties
 *     to the lowest c.  The encoder of add_with_ids and the assignment step of training.
 *   wise_pq_update: one Lloyd update; codebooks_out[j, c, :] = the mean of the sub-vectors j of the rows with codes[i, j] == c,
 *     summed in ascending row order in fp32 and divided by the count; a codeword no row chose copies codebooks_in (which must not
 *     alias codebooks_out).
 *   wise_pq_lut: lut[q, j, c] = Q[q, j-th sub-vector] . cb_jc, an index-ordered fmaf chain over dsub starting at 0.
 *   wise_pq_bias: bias[q, p] = Q[q, :] . centroids[probes[q, p], :] (0 for a probe < 0): the list's share of a row's score.
 *   wise_pq_gather_codes: out[i, :] = codes[idx[i], :] (rows of m bytes).
 *   wise_pq_find: pos[i] = the position of query_ids[i] in ids [N] (-1: absent).
 *   wise_pq_decode: out[i, :] = centroids[l, :] + concat_j cb[j, codes[pos[i], j], :] in fp32, l the list holding position pos[i]
 *     (list_off [nlist + 1]); a position outside [0, N) gives a row of NaN.  IndexIVFPQ::reconstruct_batch. */
int wise_pq_residuals(const float* x, const float* centroids, const int64_t* assign, int64_t n, int d, int nlist, float* out,
                      void* stream);
int wise_pq_encode(const float* resid, const float* codebooks, int64_t n, int d, int m, uint8_t* codes, void* stream);
int wise_pq_update(const float* resid, const uint8_t* codes, int64_t n, int d, int m, const float* codebooks_in,
                   float* codebooks_out, void* stream);
int wise_pq_lut(const float* Q, const float* codebooks, int nq, int d, int m, float* lut, void* stream);
int wise_pq_bias(const float* Q, const float* centroids, const int64_t* probes, int nq, int nprobe, int nlist, int d, float* bias,
                 void* stream);
int wise_pq_gather_codes(const uint8_t* codes, const int64_t* idx, int64_t n, int m, uint8_t* out, void* stream);
int wise_pq_find(const int64_t* ids, int64_t N, const int64_t* query_ids, int n, int64_t* pos, void* stream);
int wise_pq_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                   const float* centroids, const float* codebooks, int d, int m, float* out, void* stream);
/* The second stage of an IndexIVFPQ search (IndexIVFPQ::search behind self.index.search, src/index/feature_search_index.py:113):
 *   codes    [N,m] uint8 grouped by list (list l occupies rows list_off[l] .. list_off[l+1]-1), 16-byte aligned
 *   ids      [N] int64 external ids in the same order (NULL => the position)
 *   lut      [nq,m,256] fp32 from wise_pq_lut, 16-byte aligned;  probes [nq,nprobe] int64, entries < 0 are skipped
 *   bias     [nq,nprobe] fp32, the coarse score q . c_l of each probed list (wise_pq_bias)
 * THE ORDER OF THE ARITHMETIC IS PART OF THE CONTRACT: a row's score is acc = bias, then acc += lut[q, j, code_j] for
 * j = 0 .. m-1, in fp32, in that order — the result is reproducible bit for bit by a float32 loop on the host.
 * outD/outI as wise_ivf_scan_f32 (descending scores, (-3.4028235e38, -1) padding).  Ties: the row that comes first in codes wins.
 * Workspace: wise_ivfpq_scan_workspace_bytes(nq, nprobe, k, m) bytes (0: unsupported shape). */
size_t wise_ivfpq_scan_workspace_bytes(int nq, int nprobe, int k, int m);
int wise_ivfpq_scan(const uint8_t* codes, int64_t N, int m, const int64_t* list_off, int nlist, const int64_t* ids, const float* lut,
                    int nq, const int64_t* probes, const float* bias, int nprobe, int k, float* outD, int64_t* outI, void* workspace,
                    size_t workspace_bytes, void* stream);
/* (ABI 5, additive) wise_ivfpq_scan on ONE RANK's slice of a list-major IndexIVFPQ sharded across GPUs (rank r holds rows
 * shard_range(N_total, r, W) of the lists laid end to end; wise_amd/index/sharded.py) — what wise_ivf_scan_local_f32 is to
 * wise_ivf_scan_f32:
 *   codes, ids  [N,m] / [N] this rank's rows (ids are the global external ids);  pos_base >= 0: the position of its first row
 *   list_off    [nlist+1] the global offsets clipped to the slice (lists outside it are empty)
 *   probes, bias  [nq,nprobe] GLOBAL list numbers and their bias (the coarse stage is replicated on every rank)
 * Probes whose clipped list is empty are dropped on the device first, in probe order, together with their bias; probe_count [nq]
 * (optional) receives the number kept per query.  The kept probes are dealt evenly to as many probe groups as they fill and a
 * workgroup without a group returns before it copies the query's table, so a rank pays for the ~nprobe / W lists it holds.
 * The score's arithmetic is wise_ivfpq_scan's.  With ids == NULL outI holds pos_base + the local position (a position in the WHOLE
 * array, what wise_ivf_refine_local takes).  Ties: the row that comes first in codes wins.  wise_topk_merge of the ranks' answers
 * in rank order gives the bits of wise_ivfpq_scan over the whole array, ties included.  Limits as wise_ivfpq_scan (N is the
 * slice's).  Workspace: wise_ivfpq_scan_local_workspace_bytes(nq, nprobe, k, m) bytes (0: unsupported shape). */
size_t wise_ivfpq_scan_local_workspace_bytes(int nq, int nprobe, int k, int m);
int wise_ivfpq_scan_local(const uint8_t* codes, int64_t N, int m, const int64_t* list_off, int nlist, const int64_t* ids,
                          const float* lut, int nq, const int64_t* probes, const float* bias, int nprobe, int k, int64_t pos_base,
                          float* outD, int64_t* outI, int32_t* probe_count, void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 5, additive) The re-ranking stage of IndexIVFPQ<m>R8 / IndexIVFPQ<m>R16 (faiss IndexRefine): the candidates of a PQ scan
 * are scored again from compact copies of the rows kept in list order, and the k best are kept.
 *   rows     kind 8:  [N,d] int8 with scales [N] fp32, as wise_ip_shadow_i8 writes them (a row stands for scales[r] * rows[r,:])
 *            kind 16: [N,d] bf16 as wise_ip_shadow_bf16 writes them; scales is ignored (may be NULL).  16-byte aligned.
 *   ids      [N] int64 external ids in the same order (NULL => the position)
 *   Q        [nq,d] fp32;  cand_pos [nq,kc] int64 positions in [0, N) — what wise_ivfpq_scan returns with ids = NULL;
 *            entries outside [0, N) (the scan's -1 padding) are skipped.  A position listed twice is returned twice.
 * THE ORDER OF THE ARITHMETIC IS PART OF THE CONTRACT: with x_i = (float)rows[r,i] (kind 8: the integer's value; kind 16: the
 * bf16 bits shifted into the upper half of an fp32) a score is acc = +0, then acc = acc + (Q[q,i] * x_i) for i = 0 .. d-1 — the
 * product and the sum each rounded to fp32, never fused — and, kind 8 only, finally scales[r] * acc rounded once more.  A
 * float32 loop on the host reproduces it bit for bit.
 * outD/outI [nq,k] ordered by (-score, position), (-3.4028235e38, -1) padding where fewer than k candidates are valid.
 * Limits (WISE_E_UNSUPPORTED otherwise): kind 8: d % 16 == 0, 16 <= d <= 1024; kind 16: d % 8 == 0, 8 <= d <= 1024;
 * 1 <= kc <= 2048, 1 <= k <= 2048, nq >= 0, N < 2^32 - 1.  No workspace: one workgroup per query keeps its keys in LDS.
 *   wise_ivf_refine_rows: out[i, :] fp32 = the row the store holds at pos[i] — scales[r] * (float)rows[r,c] rounded once
 *     (kind 8), the widened bf16 (kind 16); a position outside [0, N) gives a row of NaN.  reconstruct_batch of the two types. */
int wise_ivf_refine(const void* rows, int kind, const float* scales, int64_t N, int d, const int64_t* ids, const float* Q, int nq,
                    const int64_t* cand_pos, int kc, int k, float* outD, int64_t* outI, void* stream);
int wise_ivf_refine_rows(const void* rows, int kind, const float* scales, int64_t N, int d, const int64_t* pos, int n, float* out,
                         void* stream);
/* (ABI 5, additive) wise_ivf_refine over ONE RANK's slice of the store: rows / scales / ids [N] hold positions
 * [pos_base, pos_base + N) of the whole array (pos_base >= 0).  cand_pos holds positions in the WHOLE array; an entry outside
 * [pos_base, pos_base + N) is skipped (as -1 is by wise_ivf_refine), a kept one reads local row pos - pos_base.  outD/outI ordered by
 * (-score, position); with ids == NULL the position in the whole array is written.  Same arithmetic, same limits, no workspace;
 * pos_base = 0 is wise_ivf_refine.  wise_topk_merge of the ranks' answers in rank order gives the bits of wise_ivf_refine over the
 * whole store. */
int wise_ivf_refine_local(const void* rows, int kind, const float* scales, int64_t N, int d, const int64_t* ids, const float* Q, int nq,
                          const int64_t* cand_pos, int kc, int k, int64_t pos_base, float* outD, int64_t* outI, void* stream);
/* (ABI 5, additive) IndexIVFOPQ<m>: an orthonormal rotation R [d, d] fp32 (row-major) in front of the product quantizer — faiss's
 * OPQMatrix before IndexIVFPQ.  With r = x - c_l, q . x = q . c_l + (R q) . (R r): rows are encoded from R r (wise_pq_encode) and the
 * per-query table is built from R q (wise_pq_lut); wise_pq_bias, wise_ivfpq_scan(_local) and wise_ivf_refine(_local) are unchanged.
 * Limits (WISE_E_UNSUPPORTED otherwise): d % 4 == 0, 4 <= d <= 1024, and where codes are read the wise_pq_* limits on (d, m).
 * All deterministic: the same inputs give the same bits.
 *   wise_opq_rotate: out[i, a] = sum_b x[i, b] * R[a, b] — acc = +0, then acc = fmaf(x[i, b], R[a, b], acc) for b = 0 .. d-1, in fp32,
 *     in that order, so the result depends on nothing but its inputs (not on n, the tiling or the device's load).  x [n, d], out [n, d]
 *     (must not alias x), all three 16-byte aligned.  Passing the transpose of R applies the inverse rotation.
 *   wise_opq_corr: M[a, b] = sum_i cw_i[a] * x[i, b] in fp64 (row-major [d, d] on the device), cw_i = concat_j codebooks[j, codes[i, j], :]
 *     looked up from the m code bytes of row i; x [n, d] fp32 are the UNROTATED rows.  The products are exact in fp64; the sum runs
 *     over the rows in ascending order inside blocks of 4096 rows (fma from +0), and the blocks' partial sums are then added in
 *     ascending order.  The SVD M = U S V^T gives the rotation U V^T that best maps x onto the codewords (orthogonal Procrustes).
 *     Workspace: wise_opq_corr_workspace_bytes(n, d) bytes (0: unsupported shape).
 *   wise_opq_decode: wise_pq_decode with the rotation undone — out[i, c] = centroids[l, c] + s_c, s_c = sum_a R[a, c] * cw[a] as an
 *     fmaf chain over a = 0 .. d-1 from +0 in fp32, cw = concat_j cb[j, codes[pos[i], j], :]; a position outside [0, N) gives a row
 *     of NaN.  IndexIVFOPQ::reconstruct_batch. */
int wise_opq_rotate(const float* x, const float* R, int64_t n, int d, float* out, void* stream);
size_t wise_opq_corr_workspace_bytes(int64_t n, int d);
int wise_opq_corr(const uint8_t* codes, const float* codebooks, const float* x, int64_t n, int d, int m, double* M, void* workspace,
                  size_t workspace_bytes, void* stream);
int wise_opq_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                    const float* centroids, const float* codebooks, const float* R, int d, int m, float* out, void* stream);

/* (ABI 5, additive) Search restricted to a set of ids — faiss's SearchParameters(sel = IDSelectorBatch / IDSelectorRange /
 * IDSelectorNot).  The set is resolved per index into a bitmap over row POSITIONS (rows of X; rows in list order for the
 * inverted-file indexes) and tested inside the scans, so a selective filter still returns k hits where k selected rows exist;
 * the entry points above are untouched and a search without a selector runs the kernels it ran before.
 *   wise_sel_bitmap: bit (p & 31) of bitmap[p >> 5] = 1 iff the external id of row p — ids[p], or id_base + p with ids == NULL —
 *     is selected.  mode 0: the id occurs in sel_ids [n_sel] int64, SORTED ASCENDING AND WITHOUT DUPLICATES (binary search; ids
 *     that no row carries select nothing; n_sel = 0 selects nothing); mode 1: imin <= id < imax.  invert != 0 complements the
 *     answer within the index.  bitmap has (N + 31) / 32 words, all written; the bits past N are zero, also when inverted.  One
 *     lane per row, a wave's 64 answers written by one lane from a ballot: no atomics, the same bits run after run.
 *   wise_sel_positions: pos[0 .. count) = the set positions of bitmap in ascending order, count[0] (device int64) their number
 *     (per-block popcount, scan, scatter: deterministic).  At most `capacity` entries of pos are written — capacity = N always
 *     suffices; count reports the full number either way.  Workspace: wise_sel_positions_workspace_bytes(N) bytes.
 *   wise_ip_topk_pos_f32: the fp32 scan of wise_ip_topk_f32 over the rows X[pos[i]], i < n_pos, in place of X[i] (pos ascending,
 *     entries in [0, N): what wise_sel_positions writes).  Always the single-pass VALU scan, whatever nq: every score is an fp32
 *     fmaf chain.  A selected row is one contiguous 4 d-byte burst, so the scan reads n_pos * d * 4 bytes.  Keys carry pos[i]:
 *     ties (the lower position wins), the id translation and the (-3.4028235e38, -1) padding are wise_ip_topk_f32's; n_pos == 0
 *     gives all padding.  Limits as wise_ip_topk_f32.  Workspace: wise_ip_topk_workspace_bytes(n_pos, d, nq, k) bytes.
 *   wise_ivf_scan_sel_f32: wise_ivf_scan_f32 in which only the rows whose bit of keep is set compete (same probes, same
 *     arithmetic, same ties and padding; fewer than k selected rows in the probed lists give padded slots).  A group of rows
 *     without a set bit is not loaded.  keep: (N + 31) / 32 words.  Workspace: wise_ivf_scan_workspace_bytes.
 *   wise_ivfpq_scan_sel: wise_ivfpq_scan under the same filter; the score of a selected row is the contract's — acc = bias, then
 *     acc += lut[q, j, code_j] for j ascending, in fp32 — bit for bit the unfiltered scan's score of that row, and with every bit
 *     set the output is wise_ivfpq_scan's.  With ids == NULL outI holds positions (the candidates wise_ivf_refine takes).
 *     Limits and ties as wise_ivfpq_scan.  Workspace: wise_ivfpq_scan_workspace_bytes. */
int wise_sel_bitmap(const int64_t* ids, int64_t id_base, int64_t N, int mode, const int64_t* sel_ids, int64_t n_sel, int64_t imin,
                    int64_t imax, int invert, uint32_t* bitmap, void* stream);
size_t wise_sel_positions_workspace_bytes(int64_t N);
int wise_sel_positions(const uint32_t* bitmap, int64_t N, int64_t* pos, int64_t capacity, int64_t* count, void* workspace,
                       size_t workspace_bytes, void* stream);
int wise_ip_topk_pos_f32(const float* X, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq, int k,
                         const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                         void* stream);
int wise_ivf_scan_sel_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q,
                          int nq, const int64_t* probes, int nprobe, int k, const uint32_t* keep, float* outD, int64_t* outI,
                          void* workspace, size_t workspace_bytes, void* stream);
int wise_ivfpq_scan_sel(const uint8_t* codes, int64_t N, int m, const int64_t* list_off, int nlist, const int64_t* ids,
                        const float* lut, int nq, const int64_t* probes, const float* bias, int nprobe, int k, const uint32_t* keep,
                        float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 5, additive) IndexIVFSQ8: inverted lists of 8-bit scalar-quantized rows — faiss's IndexIVFScalarQuantizer(IndexFlatIP(d), d,
 * nlist, QT_8bit, METRIC_INNER_PRODUCT), by_residual.  A row of list l is kept as d bytes, one per dimension of its residual
 * r = x - c_l (wise_pq_residuals).  trained [2 d] fp32 = vmin [d], then vdiff [d]: one range per dimension, shared by all lists.
 * Limits (WISE_E_INVALID otherwise): d % 16 == 0, 16 <= d <= 1024; the scan: k <= 2048, nprobe <= 2048, nq <= 65535.  All
 * deterministic: the same inputs give the same bits.
 *   wise_sq_train: vmin[i] = min over the n >= 1 rows of resid[:, i], vdiff[i] = max - vmin[i] (one fp32 subtraction) — faiss's
 *     RS_minmax with argument 0.  min and max are exact, so the result does not depend on the order of the rows.
 *   wise_sq_encode: codes[r, i] = clamp(floor((resid[r, i] - vmin[i]) * inv[i]), 0, 255) with inv[i] = 255 / vdiff[i] (0 where
 *     vdiff[i] == 0), the fp32 inputs widened and every operation rounded to fp64 on its own — in fp32 the roundings of the
 *     difference, the quotient and the product put values next to a bin edge into the neighbouring bin, and a value inside the
 *     trained range would no longer decode to within half a bin; values outside the trained range clamp.
 *   wise_sq_query: W[q, i] = (Q[q, i] * vdiff[i]) * (1 / 255) and q0[q] = sum_i Q[q, i] * (vmin[i] + vdiff[i] * (0.5 / 255)), every
 *     product and sum rounded on its own; the sum: lane l of 64 adds i = l, l + 64, ... in ascending order from +0, then the
 *     lanes are folded by a butterfly (v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1).  W 16-byte aligned.
 *   wise_sq_decode: out[i, c] = centroids[l, c] + (vmin[c] + ((codes[pos[i], c] + 0.5) / 255) * vdiff[c]) — faiss's Codec8bit, each
 *     operation rounded to fp32 on its own — l the list holding position pos[i] (list_off [nlist + 1]); a position outside [0, N)
 *     gives a row of NaN.  reconstruct_batch.
 *   wise_ivfsq_scan: the second stage of a search.  codes [N, d] uint8 grouped by list, 16-byte aligned; ids, probes, bias
 *     (wise_pq_bias), outD / outI, ties, padding, skipped probes and empty lists as wise_ivfpq_scan.
 *     THE ORDER OF THE ARITHMETIC IS PART OF THE CONTRACT: with C = d / 16, chunk c of a row gives s_c = +0, then
 *     s_c = fmaf(W[q, 16 c + i], (float)code[16 c + i], s_c) for i = 0 .. 15; then for step = 1, 2, 4, ... < C, at once for every
 *     c with c + step < C, s_c = s_c + s_{c + step} (the values from before the step); score = (bias[q, p] + q0[q]) + s_0, all in
 *     fp32.  tests/ivfsq_ref.py reproduces it bit for bit.  Workspace: wise_ivfsq_scan_workspace_bytes(nq, nprobe, k) bytes
 *     (0: unsupported shape); a shorter one is WISE_E_INVALID.
 *   wise_ivfsq_scan_sel: the same in which only the rows whose bit of keep ((N + 31) / 32 words over the list positions,
 *     wise_sel_bitmap) is set compete; a selected row's score is the unfiltered scan's, and with every bit set so is the output.
 *     Loads that hold no selected row are skipped. */
int wise_sq_train(const float* resid, int64_t n, int d, float* trained, void* stream);
/* (ABI 5, additive) wise_sq_train's reduction over rows that arrive in chunks, or on several ranks: lo [d] and hi [d] (device, distinct)
 * receive the per-dimension minimum and maximum of the n >= 0 rows — and of what lo / hi held before when accumulate != 0; with
 * accumulate == 0 and n == 0 they are +3.4028235e38 / -3.4028235e38, the minimum and maximum of no rows.  min and max are exact and
 * order-free: vmin = lo, vdiff = hi - lo (one fp32 subtraction) are wise_sq_train's bits over the same rows under any chunking. */
int wise_sq_minmax(const float* rows, int64_t n, int d, float* lo, float* hi, int accumulate, void* stream);
int wise_sq_encode(const float* resid, const float* trained, int64_t n, int d, uint8_t* codes, void* stream);
int wise_sq_query(const float* Q, const float* trained, int nq, int d, float* W, float* q0, void* stream);
int wise_sq_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                   const float* centroids, const float* trained, int d, float* out, void* stream);
size_t wise_ivfsq_scan_workspace_bytes(int nq, int nprobe, int k);
int wise_ivfsq_scan(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* W,
                    const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, int k, float* outD, int64_t* outI,
                    void* workspace, size_t workspace_bytes, void* stream);
int wise_ivfsq_scan_sel(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* W,
                        const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, int k, const uint32_t* keep,
                        float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 5, additive) wise_ivfsq_scan on ONE RANK's slice of a list-major IndexIVFSQ8 sharded across GPUs (rank r holds rows
 * shard_range(N_total, r, W) of the lists laid end to end; wise_amd/index/sharded.py) — what wise_ivfpq_scan_local is to
 * wise_ivfpq_scan:
 *   codes, ids  [N,d] / [N] this rank's rows (ids are the global external ids);  pos_base >= 0: the position of its first row
 *   list_off    [nlist+1] the global offsets clipped to the slice (lists outside it are empty)
 *   probes, bias  [nq,nprobe] GLOBAL list numbers and their bias;  W, q0 from wise_sq_query (the coarse stage and the ranges are
 *               replicated on every rank)
 * Probes whose clipped list is empty are dropped on the device first, in probe order, together with their bias; probe_count [nq]
 * (optional) receives the number kept per query.  The kept probes are dealt evenly to as many probe groups as they fill — one each,
 * as the whole scan gives every probe a workgroup — and a workgroup without a group returns before it loads the query's weight
 * row, so a rank pays for the ~nprobe / W lists it holds.  The score's arithmetic and its order are wise_ivfsq_scan's; a list cut
 * by a slice boundary scores its rows exactly as the whole scan does (d % 16 == 0: every slice starts 16-byte aligned, and a row's
 * chunks do not depend on where its list begins).  With ids == NULL outI holds pos_base + the local position (a position in the
 * WHOLE array).  Ties: the row that comes first in codes wins.  wise_topk_merge of the ranks' answers in rank order gives the bits
 * of wise_ivfsq_scan over the whole array, ties and padding included.  Limits and errors as wise_ivfsq_scan (N < 2^32 - 1 is the
 * slice's), and pos_base >= 0.  Workspace: wise_ivfsq_scan_local_workspace_bytes(nq, nprobe, k) bytes (0: unsupported shape); a
 * shorter one is WISE_E_INVALID.  Nothing is allocated and nothing is read back: the call can be captured into a graph. */
size_t wise_ivfsq_scan_local_workspace_bytes(int nq, int nprobe, int k);
int wise_ivfsq_scan_local(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* W,
                          const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, int k, int64_t pos_base,
                          float* outD, int64_t* outI, int32_t* probe_count, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 5, additive) range_search — faiss's Index::range_search for METRIC_INNER_PRODUCT: EVERY row with score > radius, strictly,
 * instead of the k best.  One count / fill pair per family; a hit's score is, bit for bit, the score the family's fp32 scan gives
 * that row (the same device routines in the same files): wise_ip_topk_pos_f32's single-pass VALU scan for wise_ip_range_*
 * (lane l of 64 chains fmaf over the row's float4 chunks l, l + 64, ... from +0, then a butterfly over the lane masks 32 .. 1),
 * wise_ivf_scan_f32's for wise_ivf_range_*, and the wise_ivfsq_scan contract above for wise_ivfsq_range_*.
 *   radius    finite (NaN or infinite: WISE_E_INVALID); -3.4028235e38 makes every candidate row a hit
 *   keep      optional bitmap over row positions, (N + 31) / 32 words as wise_sel_bitmap writes them: only the rows whose bit is
 *             set can be hits; a load that holds no kept row is skipped.  NULL: every row may be a hit.  (The flat count pass
 *             tests the bitmap too; it does not go through a position list.)
 *   candidates  flat: the N rows of X.  Inverted-file: the rows of the lists probes [nq, nprobe] names, entries < 0 (or >= nlist)
 *             and empty lists skipped, as in the scans; a list named twice by one query is reported twice.
 *   count     writes counts [nq] int64 (device) and leaves in the workspace what fill needs, so that the rows are read in full
 *             once: per query a hit bitmap (one bit per candidate position) and the hit count of every SEGMENT — 2048
 *             consecutive rows of X (flat), one probed list (inverted-file) — turned into exclusive offsets by a scan.
 *   fill      takes lims [nq + 1] int64 (device), the exclusive scan of counts (lims[0] = 0), the workspace count wrote and the
 *             same other arguments, and writes query q's hits to outD / outI [lims[q], lims[q + 1]) in a FIXED order: ascending
 *             position (flat); probe order, then ascending position within a list (inverted-file).  outI: ids[position], or with
 *             ids == NULL id_base + position (flat) / the position (inverted-file).  Only the hit rows are read, and their
 *             scores recomputed by the routine count used.  A caller whose counts are all 0 need not call it.
 *   order     no atomic touches global memory and none decides where a hit lands: a hit's bit is set at its row's place (an LDS
 *             OR, published as plain word stores), offsets come from popcounts and scans.  The same inputs give the same bytes.
 *   neither call allocates or reads back; both can be captured into a graph.  The caller sizes outD / outI from counts.
 * Limits, those of the family's scan: flat and wise_ivf_range_*: d % 4 == 0, 4 <= d <= 2048, X and Q 16-byte aligned;
 * wise_ivfsq_range_*: d % 16 == 0, 16 <= d <= 1024, codes and W 16-byte aligned; all: 1 <= nq <= 65535, 1 <= nprobe <= 2048,
 * 0 <= N < 2^32 - 1 (N = 0: all counts 0).  Anything else is WISE_E_INVALID with a wise_last_error text.
 * Workspace: *_range_workspace_bytes bytes (0: unsupported shape); a shorter one is WISE_E_INVALID.  It grows with nq — about
 * nq * (N / 8 + 8 * segments) bytes — so a caller with many queries runs them in chunks (wise_amd/index/range_search.py). */
size_t wise_ip_range_workspace_bytes(int64_t N, int d, int nq);
int wise_ip_range_count_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                            int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int wise_ip_range_fill_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                           int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                           size_t workspace_bytes, void* stream);
size_t wise_ivf_range_workspace_bytes(int64_t N, int nlist, int nq, int nprobe);
int wise_ivf_range_count_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                             const int64_t* probes, int nprobe, float radius, const uint32_t* keep, int64_t* counts,
                             void* workspace, size_t workspace_bytes, void* stream);
int wise_ivf_range_fill_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                            const float* Q, int nq, const int64_t* probes, int nprobe, float radius, const int64_t* lims,
                            float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
size_t wise_ivfsq_range_workspace_bytes(int64_t N, int nlist, int nq, int nprobe);
int wise_ivfsq_range_count(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const float* W,
                           const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, float radius,
                           const uint32_t* keep, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int wise_ivfsq_range_fill(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                          const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe,
                          float radius, const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                          void* stream);

/* (ABI 5, additive) IndexIVFSQfp16: inverted lists of half-precision rows — faiss's IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist,
 * QT_fp16, METRIC_INNER_PRODUCT), by_residual.  A row of list l is kept as d IEEE binary16 values (2 d bytes, little endian), one per
 * dimension of its residual r = x - c_l (wise_pq_residuals).  Nothing is trained beyond the centroids: there is no range, no weight
 * row and no q0 — the query itself is the weight.  `halves` are passed as their 16-bit patterns.  Limits, errors and determinism as
 * the wise_sq_* / wise_ivfsq_* entry points above (d % 16 == 0, 16 <= d <= 1024; k, nprobe <= 2048; nq <= 65535; halves and Q
 * 16-byte aligned).
 *   wise_sq16_encode: halves[i, c] = binary16(resid[i, c]), round to nearest even — subnormal results (|r| < 2^-14) are kept, not
 *     flushed, zeros keep their sign, |r| >= 65520 becomes +-inf: exactly numpy's float32 -> float16 cast.
 *   wise_sq16_decode: out[i, c] = centroids[l, c] + (float)halves[pos[i], c], one fp32 addition, l the list holding position pos[i];
 *     a position outside [0, N) gives a row of NaN.  reconstruct_batch.
 *   wise_ivfsq16_scan, _scan_sel, _scan_local: wise_ivfsq_scan, wise_ivfsq_scan_sel and wise_ivfsq_scan_local with the score
 *     score(row) = bias[q, p] + sum_i Q[q, i] * (float)h_i; everything else — ids == NULL, ties, padding, skipped probes, keep,
 *     pos_base, probe_count, the grids, graph capture — is theirs, from the same device code.
 *     THE ORDER OF THE ARITHMETIC IS PART OF THE CONTRACT: with C = d / 16, chunk c of a row is its elements
 *     e(c, i) = 8 c + i for i = 0 .. 7 and d / 2 + 8 c + (i - 8) for i = 8 .. 15 (the 16-byte pieces c and c + C of the row, so that
 *     a wave's 16-byte loads read contiguous runs); s_c = +0, then s_c = fmaf(Q[q, e(c, i)], (float)h[e(c, i)], s_c) for i = 0 .. 15
 *     (binary16 -> fp32 is exact, subnormals included); then for step = 1, 2, 4, ... < C, at once for every c with c + step < C,
 *     s_c = s_c + s_{c + step} (the values from before the step); score = bias[q, p] + s_0, all in fp32.  tests/ivfsqfp16_ref.py
 *     reproduces it bit for bit.  Workspaces: wise_ivfsq_scan_workspace_bytes / wise_ivfsq_scan_local_workspace_bytes.
 *   wise_ivfsq16_range_count / _fill: the count / fill pair of range_search above for this family; a hit's score is, bit for bit,
 *     wise_ivfsq16_scan's score of that row.  Workspace: wise_ivfsq_range_workspace_bytes.  As for wise_ivfsq_range_*, a list that
 *     one query names twice must come with the same bias both times (bias = q . c_l is): its hit words are kept once. */
int wise_sq16_encode(const float* resid, int64_t n, int d, uint16_t* halves, void* stream);
int wise_sq16_decode(const uint16_t* halves, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                     const float* centroids, int d, float* out, void* stream);
int wise_ivfsq16_scan(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q,
                      int nq, const int64_t* probes, const float* bias, int nprobe, int k, float* outD, int64_t* outI, void* workspace,
                      size_t workspace_bytes, void* stream);
int wise_ivfsq16_scan_sel(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                          const float* Q, int nq, const int64_t* probes, const float* bias, int nprobe, int k, const uint32_t* keep,
                          float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
int wise_ivfsq16_scan_local(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                            const float* Q, int nq, const int64_t* probes, const float* bias, int nprobe, int k, int64_t pos_base,
                            float* outD, int64_t* outI, int32_t* probe_count, void* workspace, size_t workspace_bytes, void* stream);
int wise_ivfsq16_range_count(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                             const int64_t* probes, const float* bias, int nprobe, float radius, const uint32_t* keep, int64_t* counts,
                             void* workspace, size_t workspace_bytes, void* stream);
int wise_ivfsq16_range_fill(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                            const float* Q, int nq, const int64_t* probes, const float* bias, int nprobe, float radius,
                            const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 5, additive) IndexSQfp16: exhaustive inner-product search over rows kept as IEEE binary16 — faiss's IndexScalarQuantizer(d,
 * QT_fp16, METRIC_INNER_PRODUCT) under an IndexIDMap.  The whole index is rows [N, d] binary16 bit patterns (2 d bytes a row, little
 * endian, 16-byte aligned) plus the ids: no fp32 rows and no shadow copy; the same array serves the single-query scan and, as matrix-core
 * operands as loaded, the batched passes.  Rows are encoded by wise_sq16_encode applied to the rows themselves.  Limits of every entry
 * point: d % 16 == 0, 16 <= d <= 1024, 0 <= N < 2^32 - 1, rows and Q 16-byte aligned.  Anything outside an entry point's limits, a null
 * pointer, a misaligned pointer or a workspace shorter than its *_workspace_bytes is WISE_E_INVALID with a wise_last_error text, and
 * nothing is written.  No call allocates or reads back: all can be captured into a graph.  All deterministic.
 * THE SCORE IS A CONTRACT: score(q, r) = s_0 of the wise_ivfsq16_scan arithmetic above — chunks e(c, i), one fmaf chain of 16 per
 * chunk over the exact binary16 -> fp32 conversions, the tree of adds over steps 1, 2, 4, ... — with NO bias term added (the value s_0
 * itself, a -0 included).  tests/sqfp16_flat_ref.py restates it; every entry point below returns exactly these bits.  Non-finite
 * stored values are outside the contract.  (The three workspace functions are spelled wise_ipsqfp16_*: no symbol pairs "sq16" with
 * "workspace", which the IndexIVFSQfp16 entry points established — they share the SQ8 sizes — and the tests hold.)
 *   wise_ipsq16_topk: the exact scan.  1 <= nq <= 1024, 1 <= k <= 2048; ids / id_base as wise_ip_topk_f32 (ids == NULL: id_base + row);
 *     outD descending, ties: the lower position wins, (-3.4028235e38, -1) padding when N < k; N = 0 gives all padding.  The grid runs
 *     over row ranges and a pass carries up to 4 queries; a pass reads N d 2 bytes.  Workspace: wise_ipsqfp16_topk_workspace_bytes.
 *   wise_ipsq16_topk_pos: the same scan over the rows rows[pos[i]], i < n_pos (pos ascending, entries in [0, N): what
 *     wise_sel_positions writes) — the counterpart of wise_ip_topk_pos_f32.  Keys carry pos[i]; n_pos == 0 gives all padding.
 *     Workspace: wise_ipsqfp16_topk_workspace_bytes(n_pos, d, nq, k).
 *   wise_ipsq16_range_count / _fill: the count / fill pair of range_search above over the N rows (a segment is 2048 consecutive rows;
 *     keep, radius, counts, lims, the fixed order — ascending position —, ids == NULL => id_base + position: as wise_ip_range_*);
 *     a hit iff score > radius, strictly, and a hit's score is the exact scan's, from the same device routine.  1 <= nq <= 65535.
 *     Workspace: wise_ipsqfp16_range_workspace_bytes.
 *   wise_ipsq16_reconstruct: out[i, :] = (float)rows[p, :] for the row p that carries the id query_ids[i] (ids == NULL: p = id -
 *     id_base), a row of NaN where no row does — wise_reconstruct_batch for this payload.
 *   wise_ipsq16_prepare: norms[0] (device float) = max_r |(float)rows[r, :]|_2, 0 for N = 0.  A row's norm is a fixed-order fp32 sum
 *     and the maximum is exact: the same rows give the same bits.  What the batched search's error band needs.
 *   wise_ipsq16_topk_batched: 3 or more queries in passes of 128 (d <= 512) or 64 on the matrix cores, in the threshold form of
 *     wise_ip_topk_shadow_f32's batched passes: the queries are rounded to ONE binary16 piece; per query the exact scan's k-th score
 *     over a sample of evenly spaced rows is a lower bound t of the index's exact k-th score; collect rounds on
 *     v_mfma_f32_32x32x16_f16 (the stored rows are the A operands as loaded) list EVERY (query, row) whose approximate score reaches
 *     t - eps, over growing shares of the rows first, which tightens t, then over all rows; the listed rows are re-scored by the exact
 *     scan's routine and the k best written.  eps = |q - f16(q)|_2 norms[0] (Cauchy-Schwarz on the query's rounding; the rows are not
 *     rounded again, so there is no row-side term) + d 2^-22 |q|_2 norms[0] (fp32 accumulation of both sums): no assumption on the data
 *     (DESIGN.md section 4).  A query whose list (4096 rows) overflows has its pass redone by the exact scan queued behind and gated on
 *     the device.  The answer has the bits of wise_ipsq16_topk on any data.  norms: what wise_ipsq16_prepare wrote for these rows.
 *     counters (device, two int32, may be NULL): [0] += queries answered from the lists, [1] += queries handed to the exact scan.
 *     Served: d % 128 == 0 in [256, 1024], 3 <= nq <= 1024, k <= 128, 4096 <= N < 2^31 — no floor beyond that: routing by size is the
 *     caller's.  Workspace: wise_ipsqfp16_topk_batched_workspace_bytes (0: shape not served). */
size_t wise_ipsqfp16_topk_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_ipsq16_topk(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base,
                     float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
int wise_ipsq16_topk_pos(const uint16_t* rows, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq, int k,
                         const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t wise_ipsqfp16_range_workspace_bytes(int64_t N, int d, int nq);
int wise_ipsq16_range_count(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                            int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int wise_ipsq16_range_fill(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                           int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                           void* stream);
int wise_ipsq16_reconstruct(const uint16_t* rows, int64_t N, int d, const int64_t* ids, int64_t id_base, const int64_t* query_ids,
                            int n, float* out, void* stream);
int wise_ipsq16_prepare(const uint16_t* rows, int64_t N, int d, float* norms /*[1]*/, void* stream);
size_t wise_ipsqfp16_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_ipsq16_topk_batched(const uint16_t* rows, const float* norms /*[1]*/, int64_t N, int d, const float* Q, int nq, int k,
                             const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, int32_t* counters, void* workspace,
                             size_t workspace_bytes, void* stream);

/* (ABI 5, additive) IndexSQ8bit: exhaustive inner-product search over 8-bit scalar-quantized rows — faiss's IndexScalarQuantizer(d,
 * QT_8bit, METRIC_INNER_PRODUCT) with RS_minmax (argument 0) under an IndexIDMap.  The whole index is codes [N, d] uint8 (d bytes a row,
 * 16-byte aligned), trained [2 d] fp32 (vmin [d], then vdiff [d]: wise_sq_train, or wise_sq_minmax and one subtraction) and the ids:
 * no fp32 rows and no shadow copy; the same array serves the single-query scan and, expanded in registers, the batched passes.  Rows
 * are encoded by wise_sq_encode applied to the rows themselves.  Every entry point takes the QUERIES Q [nq, d] fp32 and trained: W and
 * q0 of wise_sq_query are computed into the head of the call's workspace.  Limits of every entry point: d % 16 == 0, 16 <= d <= 1024,
 * 0 <= N < 2^32 - 1, codes, Q and the workspace 16-byte aligned.  Anything outside an entry point's limits, a null pointer, a misaligned
 * pointer or a workspace shorter than its *_workspace_bytes is WISE_E_INVALID with a wise_last_error text, and nothing is written.  No
 * call allocates or reads back: all can be captured into a graph.  All deterministic.
 * THE SCORE IS A CONTRACT: score(q, r) = q0[q] + s_0, ONE fp32 addition, with W, q0 the bits of wise_sq_query and s_0 of the
 * wise_ivfsq_scan arithmetic above — one fmaf chain of 16 per chunk from +0, the tree of adds over steps 1, 2, 4, ....  Keys, ties, the
 * range test and every returned value are on that final sum.  tests/sq8_flat_ref.py restates it; every entry point below returns exactly
 * these bits.
 *   wise_ipsq8_topk: the exact scan.  1 <= nq <= 1024, 1 <= k <= 2048; ids / id_base as wise_ip_topk_f32 (ids == NULL: id_base + row);
 *     outD descending, ties: the lower position wins, (-3.4028235e38, -1) padding when N < k; N = 0 gives all padding.  The grid runs
 *     over row ranges and a pass carries up to 4 queries; a pass reads N d bytes.  Workspace: wise_ipsq8_topk_workspace_bytes.
 *   wise_ipsq8_topk_pos: the same scan over the rows codes[pos[i]], i < n_pos (pos ascending, entries in [0, N): what
 *     wise_sel_positions writes) — the counterpart of wise_ipsq16_topk_pos.  Keys carry pos[i]; n_pos == 0 gives all padding.
 *     Workspace: wise_ipsq8_topk_workspace_bytes(n_pos, d, nq, k).
 *   wise_ipsq8_range_count / _fill: the count / fill pair of range_search above over the N rows (segments, keep, radius, counts, lims,
 *     the fixed order, ids == NULL => id_base + position: as wise_ipsq16_range_*); a hit iff score > radius, strictly, and a hit's
 *     score is the exact scan's, from the same device routine.  1 <= nq <= 65535.  The count pass leaves W and q0 in the workspace
 *     for the fill pass: both take the same workspace and queries.  Workspace: wise_ipsq8_range_workspace_bytes.
 *   wise_ipsq8_reconstruct: out[i, c] = vmin[c] + ((codes[p, c] + 0.5) / 255) * vdiff[c], each operation rounded to fp32 on its own
 *     (faiss's Codec8bit: wise_sq_decode without a centroid), for the row p that carries the id query_ids[i] (ids == NULL: p = id -
 *     id_base), a row of NaN where no row does.
 *   wise_ipsq8_prepare: norms[0] (device float) = sqrtf((float)max_r sum_c codes[r, c]^2), the largest row norm of the codes taken as
 *     the numbers 0 .. 255, 0 for N = 0.  The integer sum is exact (255^2 1024 < 2^32): the same rows give the same bits.
 *   wise_ipsq8_topk_batched: 3 or more queries in passes of 128 (d <= 512) or 64 on the matrix cores, in the threshold form of
 *     wise_ipsq16_topk_batched: sample, collect rounds, exact re-scoring, the gated exact scan behind a list that overflows.  The
 *     collect pass streams the codes, 16 to a load, expands them EXACTLY in registers to binary16 operands (every integer 0 .. 255 is
 *     a binary16 value: no row-side rounding) and issues v_mfma_f32_32x32x16_f16 against the binary16 image of 2^e W[q], e the power
 *     of two that puts the query's largest weight into [2^14, 2^15) (exact).  In that scaled space eps = |2^e W - f16(2^e W)|_2
 *     norms[0] (Cauchy-Schwarz on the image's rounding) + d 2^-22 |2^e W|_2 norms[0] (fp32 accumulation of both sums), and the threshold
 *     of a k-th score t is 2^e ((t - q0) - 2^-21 (|t| + |q0|)) - eps: the keys order fl(q0 + s_0) while the pass sees s_0 alone, and
 *     the slack pays for that addition's rounding.  A query whose weights, q0 or band are not finite, or whose
 *     largest weight is below 2^-112, hands its pass to the exact scan.  The answer has the bits of wise_ipsq8_topk on any data.
 *     norms: what wise_ipsq8_prepare wrote for these codes.  counters as wise_ipsq16_topk_batched.  Served: d % 128 == 0 in
 *     [256, 1024], 3 <= nq <= 1024, k <= 128, 4096 <= N < 2^31.  Workspace: wise_ipsq8_topk_batched_workspace_bytes (0: not served). */
size_t wise_ipsq8_topk_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_ipsq8_topk(const uint8_t* codes, const float* trained, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids,
                    int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
int wise_ipsq8_topk_pos(const uint8_t* codes, const float* trained, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q,
                        int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t wise_ipsq8_range_workspace_bytes(int64_t N, int d, int nq);
int wise_ipsq8_range_count(const uint8_t* codes, const float* trained, int64_t N, int d, const float* Q, int nq, float radius,
                           const uint32_t* keep, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int wise_ipsq8_range_fill(const uint8_t* codes, const float* trained, int64_t N, int d, const float* Q, int nq, float radius,
                          const int64_t* ids, int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                          size_t workspace_bytes, void* stream);
int wise_ipsq8_reconstruct(const uint8_t* codes, const float* trained, int64_t N, int d, const int64_t* ids, int64_t id_base,
                           const int64_t* query_ids, int n, float* out, void* stream);
int wise_ipsq8_prepare(const uint8_t* codes, int64_t N, int d, float* norms /*[1]*/, void* stream);
size_t wise_ipsq8_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_ipsq8_topk_batched(const uint8_t* codes, const float* trained, const float* norms /*[1]*/, int64_t N, int d, const float* Q,
                            int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, int32_t* counters,
                            void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 5, additive) IndexPQ<m>: exhaustive inner-product search over 8-bit product-quantizer codes kept in ROW order — faiss's
 * IndexPQ(d, m, 8, METRIC_INNER_PRODUCT) under an IndexIDMap: no lists, no centroids, no residuals.  The index is codes [N, m] uint8
 * row-major, 16-byte aligned, and the codebooks [m, 256, d / m] fp32 of the wise_pq_* entry points above, which train them, encode the
 * rows (wise_pq_encode on the rows themselves) and build the per-query tables (wise_pq_lut).
 *   lut      [nq, m, 256] fp32 exactly as wise_pq_lut writes it, 16-byte aligned: the entry points take the tables, not the queries
 *            (wise_ivfpq_scan's convention; a rotation in front would change the tables only).
 * THE SCORE IS A CONTRACT: acc = +0.0f, then acc = acc + lut[q, j, codes[r, j]] for j = 0 .. m - 1, in fp32, in that order — the bits
 * wise_ivfpq_scan gives a row of a list whose bias is +0, and the bits of tests/ivfpq_ref.scan over one list (tests/pq_flat_ref.py).
 *   wise_pqflat_topk: outD / outI [nq, k], descending scores, ties: the lower position wins, (-3.4028235e38, -1) padding when fewer
 *     than k rows compete; N = 0 gives padding only.  ids == NULL writes id_base + position (id_base = 0: the positions
 *     wise_ivf_refine takes).  nq >= 0 of any size: the call makes its own passes of 4, 2 or 1 queries, whose tables share the LDS
 *     of a workgroup; a pass reads the N m code bytes once.  Workspace: wise_pqflat_topk_workspace_bytes(N, m, nq, k).
 *   wise_pqflat_topk_pos: the same scan over the rows codes[pos[i]], i < n_pos <= N (pos ascending, entries in [0, N): what
 *     wise_sel_positions writes; an entry outside [0, N) is no row).  Keys carry pos[i], so ties go to the lower position;
 *     n_pos == 0 gives all padding.  Workspace: wise_pqflat_topk_workspace_bytes(n_pos, m, nq, k).
 *   wise_pqflat_decode: out[i, :] = concat_j codebooks[j, codes[pos[i], j], :], exact copies (wise_pq_decode without a centroid);
 *     a position outside [0, N) gives a row of NaN.  d, m as wise_pq_encode.
 * Limits: 1 <= m <= 128, 1 <= k <= 2048, 0 <= N < 2^32 - 1 (keys carry a 32-bit row): WISE_E_UNSUPPORTED / a workspace of 0 bytes
 * otherwise; a null or misaligned pointer is WISE_E_INVALID, a short workspace WISE_E_WORKSPACE, each with a wise_last_error text and
 * nothing written.  No call allocates or reads back: all can be captured into a graph.  Deterministic, no atomics on global memory. */
size_t wise_pqflat_topk_workspace_bytes(int64_t N, int m, int nq, int k);
int wise_pqflat_topk(const uint8_t* codes, int64_t N, int m, const float* lut, int nq, int k, const int64_t* ids, int64_t id_base,
                     float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
int wise_pqflat_topk_pos(const uint8_t* codes, int64_t N, int m, const int64_t* pos, int64_t n_pos, const float* lut, int nq, int k,
                         const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                         void* stream);
int wise_pqflat_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const float* codebooks, int d, int m, float* out,
                       void* stream);

/* (ABI 5, additive) IndexFlatL2: exhaustive squared-L2 search over fp32 rows — faiss's IndexFlatL2(d) under an IndexIDMap.  The index
 * is X [N, d] fp32 row-major (4 d bytes a row, 16-byte aligned), the array IndexFlatIP keeps, plus the ids.  Returned distances are
 * SQUARED L2, ascending; ties: the lower position wins; the padding when fewer than k rows compete is (+3.4028235e38, -1), faiss's L2
 * convention.  Limits of every entry point: d % 16 == 0, 16 <= d <= 1024, 0 <= N < 2^32 - 1, X and Q 16-byte aligned.  Anything
 * outside an entry point's limits, a null pointer, a misaligned pointer or a workspace shorter than its *_workspace_bytes is
 * WISE_E_INVALID with a wise_last_error text, and nothing is written.  No call allocates or reads back: all can be captured into a
 * graph.  All deterministic.
 * THE DISTANCE IS A CONTRACT.  With C = d / 16, a row is 4 C sixteen-byte pieces of four floats; chunk c = 0 .. C - 1 uses the pieces
 * c, C + c, 2 C + c and 3 C + c: element i = 0 .. 15 of the chunk is e = (i / 4) (d / 4) + 4 c + i % 4.  Start with s_c = +0; for
 * i = 0 .. 15 in order: t = q[e] - x[e], ONE rounded fp32 subtraction, then s_c = fmaf(t, t, s_c).  Then for step = 1, 2, 4, ... < C,
 * at once for every c with c + step < C: s_c = s_c + s_{c + step}.  dist(q, x) = s_0.  tests/l2_flat_ref.py restates it; every entry
 * point below returns exactly these bits.  Non-finite inputs are outside the contract.  On the device the selection runs on the
 * score -dist (negating an fp32 value is exact), so keys, ties and merges are the inner-product types'; the sign flips back on output.
 *   wise_l2_topk_f32: the exact scan.  1 <= nq <= 1024, 1 <= k <= 2048; ids / id_base as wise_ip_topk_f32 (ids == NULL: id_base + row);
 *     N = 0 gives all padding.  The grid runs over row ranges and a pass carries up to 4 queries; a pass reads N d 4 bytes, what
 *     wise_ip_topk_f32 reads.  Workspace: wise_l2_topk_workspace_bytes (0: shape not served; answers without a device).
 *   wise_l2_topk_pos_f32: the same scan over the rows X[pos[i]], i < n_pos (pos ascending, entries in [0, N): what wise_sel_positions
 *     writes) — the counterpart of wise_ipsq16_topk_pos.  Keys carry pos[i]; n_pos == 0 gives all padding.
 *     Workspace: wise_l2_topk_workspace_bytes(n_pos, d, nq, k).
 *   wise_l2_range_count_f32 / _fill_f32: the count / fill pair of range_search above over the N rows (a segment is 2048 consecutive
 *     rows; keep, counts, lims, the fixed order — ascending position —, no global atomics, ids == NULL => id_base + position: as
 *     wise_ipsq16_range_*); a hit iff dist < radius, strictly (faiss's rule for METRIC_L2), and a hit's distance is the exact scan's,
 *     from the same device routine.  1 <= nq <= 65535, radius finite.  Workspace: wise_l2_range_workspace_bytes.
 *   wise_l2_prepare: what the batched search keeps beside the rows.  Xb [N, d] bf16 and norms[0] = max_r |x_r|, norms[1] =
 *     max_r |x_r - xb_r| are wise_ip_shadow_bf16's (that entry point is called for them); half[r] (N device floats) =
 *     0.5f * |x_r|^2 as a fixed-order fp32 sum: lane l of 64 runs s = fmaf(x, x, s) from +0 over the elements of the row's
 *     16-byte pieces l, l + 64, ... in ascending order, then s = s + s[lane ^ o] for o = 32, 16, 8, 4, 2, 1, then the exact halving.
 *   wise_l2_topk_batched: 3 or more queries in passes of 128 (d <= 512) or 64 on the matrix cores, the threshold form of
 *     wise_ipsq16_topk_batched for distances.  With qb = bf16(q), |q - x|^2 / 2 = |q|^2 / 2 + |x|^2 / 2 - q . x is approximated by
 *     |q|^2 / 2 + a(r), a(r) = half[r] - qb . xb_r on v_mfma_f32_32x32x16_bf16 (the bf16 rows are the A operands as loaded).  Per
 *     query the exact scan's k-th smallest distance over a sample of evenly spaced rows is an upper bound t of the index's exact
 *     k-th distance; collect rounds list EVERY (query, row) with a(r) <= (t - |q|^2) / 2 + eps, over growing shares of the rows
 *     first, which tightens t, then over all rows; the listed rows are re-scored by the exact scan's routine and the k best
 *     written.  eps = |q - qb| norms[0] (the query's rounding) + |qb| norms[1] (the rows' rounding) + d 2^-22 |q| (norms[0] +
 *     norms[1]) (fp32 accumulation of the matrix-core sum) + d 2^-24 norms[0]^2 / 2 (the rounding of half[r]) + (d + 2) 2^-24
 *     (|q| + norms[0])^2 (the contract distance against the real one, and the threshold's own arithmetic) + a term for values
 *     below the normal range: no assumption on the data.  A query whose list (4096 rows) overflows, or whose
 *     bf16 image or eps is not finite, has its pass redone by the exact scan queued behind and gated on the device.  The answer
 *     has the bits of wise_l2_topk_f32 on any finite data.  Xb, half, norms: what wise_l2_prepare wrote for these rows.
 *     counters (device, two int32, may be NULL): [0] += queries answered from the lists, [1] += queries handed to the exact scan.
 *     Served: d % 128 == 0 in [256, 1024], 3 <= nq <= 1024, k <= 128, 4096 <= N < 2^31 — no floor beyond that: routing by size is
 *     the caller's.  Workspace: wise_l2_topk_batched_workspace_bytes (0: shape not served). */
size_t wise_l2_topk_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_l2_topk_f32(const float* X, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base, float* outD,
                     int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
int wise_l2_topk_pos_f32(const float* X, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq, int k,
                         const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t wise_l2_range_workspace_bytes(int64_t N, int d, int nq);
int wise_l2_range_count_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                            int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int wise_l2_range_fill_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids, int64_t id_base,
                           const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
int wise_l2_prepare(const float* X, int64_t N, int d, uint16_t* Xb, float* half /*[N]*/, float* norms /*[2]*/, void* stream);
size_t wise_l2_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_l2_topk_batched(const float* X, const uint16_t* Xb, const float* half, const float* norms /*[2]*/, int64_t N, int d,
                         const float* Q, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                         int32_t* counters, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 5, additive) IndexSQfp16L2: exhaustive squared-L2 search over rows stored as IEEE binary16 — faiss's IndexScalarQuantizer(d,
 * QT_fp16, METRIC_L2) under an IndexIDMap, the L2 twin of IndexSQfp16.  The index is rows [N, d] binary16 row-major (2 d bytes a row,
 * 16-byte aligned; the bits wise_sq16_encode writes, as IndexSQfp16 stores them) plus the ids: N (2 d + 8) bytes, no fp32 rows and no
 * second copy of the rows.  Returned distances are SQUARED L2, ascending; ties: the lower position wins; the padding when fewer than
 * k rows compete is (+3.4028235e38, -1).  Limits of every entry point are IndexSQfp16's: d % 16 == 0, 16 <= d <= 1024,
 * 0 <= N < 2^32 - 1, rows and Q 16-byte aligned.  Anything outside an entry point's limits, a null pointer, a misaligned pointer or a
 * workspace shorter than its *_workspace_bytes is WISE_E_INVALID with a wise_last_error text, and nothing is written.  No call
 * allocates or reads back: all can be captured into a graph.  All deterministic; no packed-f32 math.
 * THE DISTANCE IS A CONTRACT.  With C = d / 16, chunk c = 0 .. C - 1 of a row is the chunk of the wise_ivfsq16_scan arithmetic: the
 * elements 8 c .. 8 c + 7 (i = 0 .. 7) and d / 2 + 8 c .. d / 2 + 8 c + 7 (i = 8 .. 15).  Start with s_c = +0; for i = 0 .. 15 in
 * order: t = q[e] - (float)h[e], ONE rounded fp32 subtraction (the widening is exact, subnormals are kept), then s_c = fmaf(t, t, s_c).
 * Then for step = 1, 2, 4, ... < C, at once for every c with c + step < C: s_c = s_c + s_{c + step}.  dist(q, h) = s_0.
 * tests/sqfp16_l2_ref.py restates it; every entry point below returns exactly these bits.  Non-finite inputs are outside the
 * contract.  On the device the selection runs on the score -dist, as for IndexFlatL2; the sign flips back on output.
 *   wise_l2sq16_topk: the exact scan.  1 <= nq <= 1024, 1 <= k <= 2048; ids / id_base as wise_ip_topk_f32 (ids == NULL: id_base + row);
 *     N = 0 gives all padding.  The grid runs over row ranges and a pass carries up to 4 queries; a pass reads N d 2 bytes.
 *     Workspace: wise_l2sqfp16_topk_workspace_bytes (0: shape not served; answers without a device).
 *   wise_l2sq16_topk_pos: the same scan over the rows rows[pos[i]], i < n_pos (pos ascending, entries in [0, N): what
 *     wise_sel_positions writes).  Keys carry pos[i]; n_pos == 0 gives all padding.
 *     Workspace: wise_l2sqfp16_topk_workspace_bytes(n_pos, d, nq, k).
 *   wise_l2sq16_range_count / _fill: the count / fill pair of range_search above over the N rows (segments, keep, counts, lims, the
 *     fixed order — ascending position —, ids == NULL => id_base + position: as wise_ipsq16_range_*; no atomic touches global
 *     memory); a hit iff dist < radius, strictly, and a hit's distance is the exact scan's, from the same device routine.
 *     1 <= nq <= 65535, radius finite.  Workspace: wise_l2sqfp16_range_workspace_bytes.
 *   wise_l2sq16_prepare: ALL the batched search keeps beside the rows, N 4 bytes.  half[r] (N device floats) = 0.5f * sum (float)h^2
 *     as a fixed-order fp32 sum, wise_l2_prepare's order over pieces of 8 halves: lane l of 64 runs s = fmaf(x, x, s) from +0 over the
 *     widened elements of the row's 16-byte pieces l, l + 64 in ascending order, then s = s + s[lane ^ o] for o = 32, 16, 8, 4, 2, 1,
 *     then the exact halving.  norms[0] (one device float) = sqrtf(2 max_r half[r]): the largest row norm max_r |h_r|, 0 for N = 0
 *     (one block folds the half-norms: a maximum is exact in any order, no atomic).
 *   wise_l2sq16_topk_batched: 3 or more queries in passes of 128 (d <= 512) or 64 on the matrix cores: wise_l2_topk_batched in its
 *     threshold form — sample, collect rounds, exact re-scoring, the gated exact scan behind a list (4096 rows) that overflows (a
 *     list is appended to through its counter, in any order: the re-scoring keys carry the row) — where the collect operand is the
 *     stored binary16 row AS LOADED on v_mfma_f32_32x32x16_f16 against q16 = f16(q): there is no bf16 copy.  a(r) = half[r] - q16 . h_r
 *     approximates (dist - |q|^2) / 2, and eps is wise_l2_topk_batched's term by term with the rows' rounding term gone (the rows are
 *     exact operands): |q - q16| norms[0] (the query's rounding) + d 2^-22 |q| norms[0] (fp32 accumulation) + d 2^-24 norms[0]^2 / 2
 *     (the rounding of half[r]) + (d + 2) 2^-24 (|q| + norms[0])^2 (the contract distance against the real one, and the threshold's
 *     own arithmetic) + a term for values below the normal range.  A query whose binary16 image (a component
 *     beyond 65504) or eps is not finite hands its pass to the exact scan.  The answer has the bits of wise_l2sq16_topk on any finite
 *     data.  half, norms: what wise_l2sq16_prepare wrote for these rows.  counters as wise_l2_topk_batched.  Served:
 *     d % 128 == 0 in [256, 1024], 3 <= nq <= 1024, k <= 128, 4096 <= N < 2^31.
 *     Workspace: wise_l2sqfp16_topk_batched_workspace_bytes (0: shape not served).
 * reconstruct_batch over these rows is wise_ipsq16_reconstruct. */
size_t wise_l2sqfp16_topk_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_l2sq16_topk(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base,
                     float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream);
int wise_l2sq16_topk_pos(const uint16_t* rows, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq, int k,
                         const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t wise_l2sqfp16_range_workspace_bytes(int64_t N, int d, int nq);
int wise_l2sq16_range_count(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                            int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int wise_l2sq16_range_fill(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                           int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                           void* stream);
int wise_l2sq16_prepare(const uint16_t* rows, int64_t N, int d, float* half /*[N]*/, float* norms /*[1]*/, void* stream);
size_t wise_l2sqfp16_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k);
int wise_l2sq16_topk_batched(const uint16_t* rows, const float* half, const float* norms /*[1]*/, int64_t N, int d, const float* Q,
                             int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, int32_t* counters,
                             void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 5, additive) IndexIVFFlatL2: inverted-file search under squared L2 — faiss's IndexIVFFlat(IndexFlatL2(d), d, nlist, METRIC_L2).
 * The lists hold the raw fp32 rows X [N, d] grouped by list (no residual), 4 d bytes a row.  Limits are IndexFlatL2's: d % 16 == 0,
 * 16 <= d <= 1024, X and Q 16-byte aligned, 0 <= N < 2^32 - 1; and k <= 2048, nprobe <= 2048, nq <= 65535.  Anything else, a null
 * pointer or a short workspace is WISE_E_INVALID with a wise_last_error text, and nothing is written.  No call allocates or reads
 * back: every call can be captured into a graph.  All deterministic.
 * THE DISTANCE IS THE CONTRACT OF wise_l2_topk_f32 ABOVE: a row of a list scores, bit for bit, what IndexFlatL2 gives the same (query,
 * row) — the same device routine.  Selection runs on -dist (exact), so keys, ties (the row that comes first in X wins), the merge of the
 * probed lists and wise_topk_merge are the inner-product types'.  Outputs are squared distances, ascending, padded with
 * (+3.4028235e38, -1).
 *   wise_ivfl2_scan: arguments as wise_ivf_scan_f32.  Probes < 0 or >= nlist are skipped, and so are empty lists.  One block per
 *     (query, probe), the list kernels of wise_ivfsq16_scan over fp32 rows.  Workspace: wise_ivfl2_scan_workspace_bytes(nq, nprobe, k).
 *   wise_ivfl2_scan_sel: the same with keep, (N + 31) / 32 words as wise_sel_bitmap writes them: only the rows whose bit is set compete;
 *     a selected row's distance is the unfiltered scan's, and with every bit set the output is the unfiltered scan's.
 *   wise_ivfl2_scan_local: the rank-local form for a slice of the list-major array, as wise_ivfsq16_scan_local: list_off clipped to
 *     the slice, pos_base >= 0 the position of the slice's first row, probes whose list is empty in the slice dropped first (in probe
 *     order; probe_count [nq], optional, receives the number kept), group-major block order, and with ids == NULL outI = pos_base +
 *     row.  wise_topk_merge of the ranks' NEGATED answers in rank order gives, negated back, the bits of wise_ivfl2_scan over the
 *     whole array.  Workspace: wise_ivfl2_scan_local_workspace_bytes(nq, nprobe, k).
 *   wise_ivfl2_range_count / _fill: the count / fill pair of range_search above over the probed lists; a hit iff dist < radius,
 *     strictly; fixed order: probe order, then ascending position; keep optional; radius finite; a hit's distance is the scan's.
 *     Workspace: wise_ivfl2_range_workspace_bytes(N, nlist, nq, nprobe).
 * THE COARSE RULE IS A CONTRACT: g(x, c) = fl(s(x, c) - h_c), where s is wise_ip_scores_f32's index-ordered fmaf chain from +0 and
 * h_c = 0.5f * |c|^2 is wise_l2_half_norms's value (|x - c|^2 = |x|^2 - 2 (x . c - |c|^2 / 2): the largest g is the nearest
 * centroid).  A row goes to argmax_c g, ties to the lowest c (wise_ivf_argmax); a query probes the nprobe largest g
 * (wise_select_topk_f32, -1 padding when nprobe > nlist).  Assignment and probing use the same arithmetic, so a stored row's own list
 * is among its probes at any nprobe >= 1.
 *   wise_l2_half_norms: half[r] = 0.5f * |x_r|^2, exactly wise_l2_prepare's (the same kernel); N = 0 writes nothing.
 *   wise_ivf_l2_coarse: in place, scores[r, c] = scores[r, c] - half[c] for scores [rows, nlist]: one rounded fp32 subtraction.
 *   wise_ivf_list_means: out[c, :] = sums[c, :] / (float)counts[c], one correctly rounded fp32 division per element (counts int64, as
 *     wise_ivf_group writes them); rows with count 0 are left as they are; out may be sums.  The plain k-means update. */
size_t wise_ivfl2_scan_workspace_bytes(int nq, int nprobe, int k);
int wise_ivfl2_scan(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q, int nq,
                    const int64_t* probes, int nprobe, int k, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                    void* stream);
int wise_ivfl2_scan_sel(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q, int nq,
                        const int64_t* probes, int nprobe, int k, const uint32_t* keep, float* outD, int64_t* outI, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t wise_ivfl2_scan_local_workspace_bytes(int nq, int nprobe, int k);
int wise_ivfl2_scan_local(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q,
                          int nq, const int64_t* probes, int nprobe, int k, int64_t pos_base, float* outD, int64_t* outI,
                          int32_t* probe_count, void* workspace, size_t workspace_bytes, void* stream);
size_t wise_ivfl2_range_workspace_bytes(int64_t N, int nlist, int nq, int nprobe);
int wise_ivfl2_range_count(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                           const int64_t* probes, int nprobe, float radius, const uint32_t* keep, int64_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream);
int wise_ivfl2_range_fill(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q,
                          int nq, const int64_t* probes, int nprobe, float radius, const int64_t* lims, float* outD, int64_t* outI,
                          void* workspace, size_t workspace_bytes, void* stream);
int wise_l2_half_norms(const float* X, int64_t N, int d, float* half /*[N]*/, void* stream);
int wise_ivf_l2_coarse(float* scores, const float* half, int rows, int nlist, void* stream);
int wise_ivf_list_means(const float* sums, const int64_t* counts, int nlist, int d, float* out, void* stream);

/* (ABI 5, additive) remove_ids — stable, in-place compaction of an index's per-row arrays under a bitmap over row positions.
 *   keep      (N + 31) / 32 words as wise_sel_bitmap writes them, bit p set = row p STAYS.  The bits past N are ignored, whatever
 *             they hold.
 *   plan      wise_compact_plan_entries(N) = ceil(N / 2048) + 1 int64 (device), written by wise_compact_plan: plan[s] = the number
 *             of kept rows before row 2048 s; the last entry is the total, which also goes to count[0] (device int64).
 *   rank      out[i] = the number of kept rows strictly before position pos[i], 0 <= pos[i] <= N (values outside are clamped):
 *             list_off [nlist + 1] becomes the offsets after the removal in one launch.  pos and out may be the same array.
 *   rows      the kept rows of data [N, width_bytes] (row-major, no padding) move to rows 0 .. kept - 1 in their order, in
 *             place; what lies behind them afterwards is unspecified.  The only other memory written is scratch: the array is
 *             worked through in ascending chunks of scratch_bytes / width_bytes rows (whole multiples of 2048 when more than
 *             2048 fit), each gathered into the scratch and then copied down, in two launches, so that every source of a chunk
 *             is read before any of its destinations is written; a chunk whose destinations all lie below it is written in
 *             place, and a chunk in front of the first removed row is left alone.  1 <= width_bytes <= 65536; accesses are 16
 *             bytes wide when width_bytes, data and scratch are multiples of 16, else the largest power of two dividing all three.
 *             The same plan serves every array of the index (payload, ids, compact rows, scales).
 * No atomic decides where a row lands (ranks are popcounts and scans), so the same inputs give the same bytes.  Nothing is
 * allocated and nothing is read back: all three calls can be captured into a graph.  0 <= N < 2^32 - 1; N = 0, keep-all and
 * keep-none are valid.  A scratch smaller than one row, a null pointer or a size out of range is WISE_E_INVALID with a
 * wise_last_error text. */
int64_t wise_compact_plan_entries(int64_t N);
int wise_compact_plan(const uint32_t* keep, int64_t N, int64_t* plan, int64_t* count, void* stream);
int wise_compact_rank(const uint32_t* keep, int64_t N, const int64_t* plan, const int64_t* pos, int64_t n, int64_t* out,
                      void* stream);
int wise_compact_rows(void* data, int64_t N, int64_t width_bytes, const uint32_t* keep, const int64_t* plan, void* scratch,
                      size_t scratch_bytes, void* stream);

/* Merge `parts` partial top-k lists (e.g. one per GPU after the RCCL all-gather) into one.
 * inD [parts,nq,k] fp32, inI [parts,nq,k] int64 (entries with id -1 are padding) -> outD/outI [nq,k].
 * Ties: lower part index first, then the order within the part.  k <= 2048, parts*k <= 65536. */
int wise_topk_merge(const float* inD, const int64_t* inI, int parts, int nq, int k, float* outD,
                    int64_t* outI, void* stream);

/* IndexIDMap::reconstruct_batch (api/routes.py:1078): out[i,:] = X[row_of(ids_query[i]),:].
 * ids==NULL => row = id - id_base.  With ids given, a linear search kernel maps id -> row
 * (faiss does the same without a direct map).  Missing ids give a row of NaN. */
int wise_reconstruct_batch(const float* X, int64_t N, int d, const int64_t* ids, int64_t id_base,
                           const int64_t* query_ids, int n, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HP-1  OpenCLIP VisionTransformer image tower (replaces model.encode_image + L2 normalise,
 *       reference call site src/feature/mlfoundation_openclip.py:99-100)
 *
 * Weights are two caller-owned device blobs in the fixed layout wise_vit_layout() reports:
 *   wb  bf16 : conv1 [W, Kp] (K = 3*P*P zero-padded to Kp = roundup(K,64)), then per layer
 *              in_proj [3W,W], out_proj [W,W], c_fc [F,W], c_proj [W,F], then proj^T [D,W]
 *   pf  fp32 : class_embedding [W], positional_embedding [T,W], ln_pre w,b [W],[W], then per layer
 *              ln_1 w,b, in_proj_bias [3W], out_proj bias [W], ln_2 w,b, c_fc bias [F], c_proj bias [W],
 *              then ln_post w,b
 * (names are open_clip 2.24.0 state-dict keys under `visual.`; see wise_amd/feature/vit_weights.py)
 * ---------------------------------------------------------------------------------------------- */
typedef struct wise_vit_config {
    int32_t image_size; /* S: 224 */
    int32_t patch;      /* P: 32 (ViT-B/32), 14 (ViT-L/14), 16 */
    int32_t width;      /* W: 768 / 1024 ; multiple of 128, head dim must be 64 */
    int32_t layers;     /* L */
    int32_t heads;      /* H = W/64 */
    int32_t mlp;        /* F: 4W */
    int32_t embed_dim;  /* D: 512 / 768 */
    int32_t act;        /* 0 = QuickGELU x*sigmoid(1.702x) (openai tags), 1 = erf GELU, 2 = GELU tanh form */
    int32_t arch;       /* 0 = open_clip VisionTransformer (class token, ln_pre, ln_post on the class row, linear projection);
                           1 = timm ViT as open_clip's SigLIP towers use it (`TimmModel`, pool 'map'): no class token, no
                           ln_pre, LayerNorm eps 1e-6, final norm over all tokens, attention-pool head (one latent query,
                           projection, y + mlp(norm(y))), no projection (embed_dim == width); u8 input is normalised with
                           mean = std = 0.5.  Weight layout of arch 1: wise_amd/feature/siglip.py:pack_siglip_vision */
    int32_t ln_fold;    /* (ABI 5) 0 = LayerNorm kernels between the GEMMs; 1 (arch 0 only) = the blocks' LayerNorms folded into
                           the GEMMs around them: the residual stream is kept as bf16 hi + lo, the residual GEMMs also emit the
                           rows' 1/sqrt(var + eps), the QKV / fc1 GEMMs take hi as their operand and scale their rows by it.  The blob layout is the same, but the packer must then store
                           in_proj / c_fc as gamma-scaled, row-centred weights and their biases as b + W beta
                           (wise_amd/feature/vit.py:pack_weights); ln_1 / ln_2 slots are not read.  Same results within the
                           bf16 path's tolerance (not bit-equal to ln_fold = 0).
                           2 = 1 with a block's attention, out-projection, residual add and row statistics in ONE kernel
                           (wise_attention_oproj_fold: up to 64 tokens, 12 heads of 64 — ViT-B/32); bit-equal to ln_fold = 1. */
} wise_vit_config;

#define WISE_VIT_IN_F32 0  /* images [B,3,S,S] fp32, already normalised (preprocess_image output) */
#define WISE_VIT_IN_U8 1   /* images [B,3,S,S] uint8 0..255; (x/255-mean)/std fused in the patch gather */

/* element counts of the two blobs and the byte offset table (for packers); returns 0 or WISE_E_* */
int wise_vit_layout(const wise_vit_config* cfg, int64_t* wb_elems, int64_t* pf_elems);
size_t wise_vit_workspace_bytes(const wise_vit_config* cfg, int batch);
/* out [B,D] fp32, rows L2-normalised without epsilon (mlfoundation_openclip.py:100). */
int wise_vit_forward(const wise_vit_config* cfg, const uint16_t* wb, const float* pf,
                     const void* images, int in_kind, int batch, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same forward kept entirely on `stream` (wise_vit_forward splits a batch of >= 64 images into two halves on two
 * internal streams).  For callers that pipeline whole batches themselves — two in flight, each with its own stream and
 * workspace; workspace_bytes as reported by wise_vit_workspace_bytes. */
int wise_vit_forward_single(const wise_vit_config* cfg, const uint16_t* wb, const float* pf, const void* images,
                            int in_kind, int batch, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Debug/parity tap: copy the residual stream x [B*T, W] fp32 as it stands after `after_layer`
 * blocks (0 = after ln_pre) from the workspace of the LAST forward into dst.  With ln_fold != 0 and
 * head dim 64 the last block's MLP (ln_fold = 1: also its attention half) runs for the class rows
 * only: those rows hold the last block's output; every other row holds block L-2's output
 * (ln_fold = 1), or that plus the last block's attention residual (ln_fold = 2). */
int wise_vit_tap_residual(const wise_vit_config* cfg, int batch, const void* workspace, float* dst,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * HP-1 audio  MS-CLAP (version 2023) HTSAT audio encoder + projection (replaces
 *       self.model.clap.audio_encoder(x)[0] + L2 normalise, reference call site
 *       src/feature/microsoft_clap.py:49-50).  The architecture is fixed (msclap config_2023:
 *       n_fft 1024, hop 320, 64 mel bands 50..8000 Hz at sr 44100, Swin depths 2-2-6-2, dims 96..768,
 *       heads 4..32, window 8, projection 768->1024), so there is no config struct.
 * wave [B, samples] fp32 (what preprocess_audio yields after the reshape at microsoft_clap.py:47-48);
 * only the first 1024 STFT frames (6.8 s at hop 320) enter the model.  out [B,1024] fp32, unit rows.
 * Weight blobs: layout in wise_amd/feature/htsat.py:pack_htsat_weights (msclap state-dict keys).
 * ---------------------------------------------------------------------------------------------- */
int wise_htsat_layout(int64_t* wb_elems, int64_t* pf_elems);
size_t wise_htsat_workspace_bytes(int batch, int samples);
int wise_htsat_forward(const uint16_t* wb, const float* pf, const float* wave, int batch, int samples,
                       float* out, void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 5) wise_htsat_forward with flags.  bit 0: the LayerNorms of stages 2 - 4 folded into the GEMMs around them (the
 * residual stream of those stages as bf16 hi + lo; see wise_gemm_fold_resid) — the packer must then store the folded qkv / fc1
 * weights and biases of those stages (wise_amd/feature/htsat.py:pack_htsat_weights(fold=True)).  bit 1: the MLP of every block
 * of stages 2 and 3 through wise_mlp_stream (one kernel, hidden activations in registers) — the packer must then store those
 * blocks' fc1 + fc2 slots as that kernel's weight stream (pack_htsat_weights(mlp_stream=True)).  bit 2: norm1 + QKV projection
 * + window attention of every block of stages 2 and 3 through wise_swin_qkv_attn — the packer must then store those blocks'
 * qkv weight and bias slots as that kernel's stream (pack_htsat_weights(attn_stream=True)).  Bit 0 excludes bits 1 and 2.
 * flags 0 = wise_htsat_forward. */
int wise_htsat_forward2(const uint16_t* wb, const float* pf, const float* wave, int batch, int samples,
                        float* out, void* workspace, size_t workspace_bytes, int flags, void* stream);
/* parity tap after a forward with the same (batch, samples): what 0 = BatchNorm'd log-mel
 * [B*frames,64], 1 = residual stream (fp32 rows), 2 = the last stage's residual stream of a flags-bit-0 forward (hi + lo,
 * returned as fp32); copies `count` floats. */
int wise_htsat_tap(int what, const void* workspace, int batch, int samples, float* dst, int64_t count,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * HP-1 audio  MS-CLAP (version 2022) audio encoder: PANNs Cnn14 + projection — the same reference call site
 *       (src/feature/microsoft_clap.py:49-50) when the feature id's version token is '2022'
 *       (:20-31: every key of msclap's CLAP.model_name is accepted).  Fixed architecture (msclap config_2022:
 *       n_fft 1024, hop 320, 64 mel bands 50..14000 Hz at sr 44100; six ConvBlocks 64..2048 channels of two
 *       3x3 convolutions + BatchNorm + ReLU, 2x2 average pooling after the first five; mean over mel, max + mean over
 *       time; fc1 2048->2048 + ReLU; projection 2048->1024).  wave [B, samples] fp32, any length of at least 32 STFT
 *       frames (the whole clip enters the model).  out [B,1024] fp32, unit rows.
 * Weight blobs: layout in wise_amd/feature/cnn14.py:pack_cnn14_weights (msclap state-dict keys; BatchNorm folded).
 * ---------------------------------------------------------------------------------------------- */
int wise_cnn14_layout(int64_t* wb_elems, int64_t* pf_elems);
size_t wise_cnn14_workspace_bytes(int batch, int samples);
int wise_cnn14_forward(const uint16_t* wb, const float* pf, const float* wave, int batch, int samples,
                       float* out, void* workspace, size_t workspace_bytes, void* stream);
/* parity tap after a forward with the same (batch, samples): what 0 = BatchNorm'd log-mel fp32 [B*frames*64],
 * 1 = pooled latent bf16 [B*2048], 2 = fc1 output bf16 [B*2048]; copies `bytes` bytes. */
int wise_cnn14_tap(int what, const void* workspace, int batch, int samples, void* dst, int64_t bytes,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * HP-2 query side: OpenCLIP text tower — replaces `self.model.encode_text(tokens)` + L2
 *       normalise, reference call site src/feature/mlfoundation_openclip.py:103-108 (reached from
 *       FeatureSearchIndex.search, src/index/feature_search_index.py:112).  Token ids in, unit vectors out;
 *       tokenising stays on the host (wise_amd/feature/clip_tokenizer.py).
 *
 *   wb  bf16 : per layer in_proj [3W,W], out_proj [W,W], c_fc [F,W], c_proj [W,F]; then text_projection^T [D,W]
 *   pf  fp32 : token_embedding [V,W], positional_embedding [T,W]; per layer ln_1 w,b, in_proj_bias [3W],
 *              out_proj bias [W], ln_2 w,b, c_fc bias [F], c_proj bias [W]; then ln_final w,b
 * (open_clip 2.24.0 state-dict keys without the `visual.` prefix; see wise_amd/feature/text.py)
 * tokens int32 [batch, context] (device): <start_of_text> ... <end_of_text> 0 0 ...; the pooled row is
 * argmax(tokens[b]) as in open_clip (the end-of-text id is the largest id of the vocabulary).
 * The MS-CLAP caption encoder (src/feature/microsoft_clap.py:53-58: GPT-2 base + msclap Projection) is the same
 * pipeline with act = 2, pool = 1, head = 1; then wb ends with W1 [1024,W], W2 [1024,1024] and pf with the
 * Projection's LayerNorm w,b [1024] after ln_f.
 * ---------------------------------------------------------------------------------------------- */
typedef struct wise_text_config {
    int32_t context;    /* T: 77 */
    int32_t vocab;      /* V: 49408 */
    int32_t width;      /* W: 512 (ViT-B/32), 768 (ViT-L/14); multiple of 128, head dim 64 */
    int32_t layers;     /* L: 12 */
    int32_t heads;      /* H = W/64 */
    int32_t mlp;        /* F = 4W */
    int32_t embed_dim;  /* D: 512 / 768 (1024 with head = 1) */
    int32_t act;        /* 0 = QuickGELU, 1 = erf GELU, 2 = gelu_new (tanh form, GPT-2) */
    int32_t pool;       /* pooled row: 0 = first argmax of the ids (open_clip), 1 = last id != 0 (msclap, pad id 0),
                           2 = the last position of the context (open_clip pool_type 'last': SigLIP) */
    int32_t head;       /* 0 = ln_final + linear projection; 1 = ln_f + msclap Projection (W1, GELU, W2, LayerNorm);
                           2 = ln_final + Linear WITH bias (SigLIP: pf ends with the bias [D] after ln_final w,b) */
    int32_t no_causal;  /* 0 = causal mask (CLIP, GPT-2); 1 = none (open_clip no_causal_mask: SigLIP) */
    int32_t eps_e6;     /* LayerNorm epsilon: 0 = 1e-5, 1 = 1e-6 (SigLIP norm_kwargs) */
} wise_text_config;
int wise_text_layout(const wise_text_config* cfg, int64_t* wb_elems, int64_t* pf_elems);
size_t wise_text_workspace_bytes(const wise_text_config* cfg, int batch);
int wise_text_forward(const wise_text_config* cfg, const uint16_t* wb, const float* pf, const int32_t* tokens,
                      int batch, float* out /* [batch, D] fp32, L2-normalised */, void* workspace,
                      size_t workspace_bytes, void* stream);
/* parity tap: residual stream fp32 [batch*context, W] of the last forward with the same batch */
int wise_text_tap_residual(const wise_text_config* cfg, int batch, const void* workspace, float* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HP-2 query side for open_clip models whose text tower wraps a Hugging Face encoder (`HFTextEncoder`):
 *       XLM-RoBERTa with the mean pooler and the two-layer MLP projection — the text tower of
 *       xlm-roberta-large-ViT-H-14/frozen_laion5b_s13b_b90k, the reference's DEFAULT feature id
 *       (extract-features.py:192; reached from src/feature/mlfoundation_openclip.py:103-108 like wise_text_forward).
 *       tokens int32 [batch, context], right-padded with pad_id (the HF tokenizer's padding='max_length').
 * Weight layout (host packer: wise_amd/feature/xlmr_text.py):
 *   wb bf16: per layer  W_qkv [3W,W] (query|key|value), W_out [W,W], W_fc1 [F,W], W_fc2 [W,F];  then the projection
 *            W_p1 [Hd,W], W_p2 [D,Hd]  (open_clip 'mlp' proj, Hd = (W + D)/2, no biases)
 *   pf fp32: word_emb [V,W], pos_emb [P,W], type_emb row 0 [W], embedding LayerNorm w,b;  per layer  b_qkv [3W],
 *            b_out [W], attention-output LayerNorm w,b, b_fc1 [F], b_fc2 [W], output LayerNorm w,b
 * ---------------------------------------------------------------------------------------------- */
typedef struct wise_xlmr_config {
    int32_t context;        /* T: 77 (open_clip's context_length) */
    int32_t vocab;          /* V: 250002 */
    int32_t max_positions;  /* P: 514 */
    int32_t width;          /* W: 1024; multiple of 128, head dim 64 */
    int32_t layers;         /* L: 24 */
    int32_t heads;          /* H = W/64 */
    int32_t mlp;            /* F: 4096 */
    int32_t proj_hidden;    /* Hd: (W + D)/2 */
    int32_t embed_dim;      /* D: 1024 */
    int32_t pad_id;         /* 1 (XLM-R <pad>); 0 for BERT's [PAD] */
    /* ABI 4: the BERT-family switches (all 0 = XLM-RoBERTa under open_clip's HFTextEncoder) */
    int32_t pos_mode;       /* 0: position = cumsum(mask)*mask + pad (RoBERTa); 1: position = 0..T-1 (BERT) */
    int32_t pool;           /* 0: mean over the sequence's own tokens; 1: the first row ([CLS]) */
    int32_t head;           /* 0: W -> Hd -> D, GELU between, no biases (open_clip 'mlp'); 1: msclap Projection
                             *    (e1 = W1 x, e2 = W2 gelu(e1), LayerNorm(e1 + e2); Hd = D = 1024; the fp32 blob then
                             *    ends with that LayerNorm's w, b [D]) — MS-CLAP 2022's caption encoder */
    int32_t eps_e12;        /* LayerNorm eps in units of 1e-12 (BERT: 1); 0 = 1e-5 */
} wise_xlmr_config;
int wise_xlmr_layout(const wise_xlmr_config* cfg, int64_t* wb_elems, int64_t* pf_elems);
size_t wise_xlmr_workspace_bytes(const wise_xlmr_config* cfg, int batch);
int wise_xlmr_forward(const wise_xlmr_config* cfg, const uint16_t* wb, const float* pf, const int32_t* tokens,
                      int batch, float* out /* [batch, D] fp32, L2-normalised */, void* workspace,
                      size_t workspace_bytes, void* stream);
/* parity tap: residual stream fp32 [batch*context, W] of the last forward with the same batch */
int wise_xlmr_tap_residual(const wise_xlmr_config* cfg, int batch, const void* workspace, float* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HP-1  image transform on the GPU: replaces the per-frame CPU loop of
 *       MlfoundationOpenClip.preprocess_image, src/feature/mlfoundation_openclip.py:81-90, for uint8 frames
 *       [n,3,H,W] (the decoder's output, src/dataloader/dataset.py:298):
 *       to_pil_image -> Resize(S, BICUBIC, shorter side) -> CenterCrop(S)   => uint8 [n,3,S,S],
 *       bit-identical to Pillow's 8-bit antialiased resampler; ToTensor + Normalize happen inside
 *       wise_vit_forward(in_kind = WISE_VIT_IN_U8).
 *
 * A plan belongs to one (H, W, S).  plan_init and tables are host-only (no GPU needed); the caller copies the
 * `table_bytes` blob to the device once and passes it to every wise_preproc_u8 call for that geometry.
 * Limits: H, W <= 16384; S % 4 == 0; the staged input of one output tile must fit 64 KiB of LDS
 * (downscale factors up to ~20x).
 * ---------------------------------------------------------------------------------------------- */
typedef struct wise_preproc_plan {
    int32_t H, W, S;            /* input frame size, output edge */
    int32_t new_w, new_h;       /* size after Resize(S) (torchvision: long side = int(S*long/short)) */
    int32_t left, top;          /* CenterCrop origin inside the resized image */
    int32_t tile;               /* output tile edge of one workgroup */
    int32_t ndh, ndv;           /* dwords of padded taps per output column / row */
    int32_t max_cols4, max_rows4; /* staged input rectangle of the worst tile: column dwords, rows / 4 */
    int32_t lds_bytes;
    int32_t reserved;           /* bit 0 (set by the _init functions): 0 = Resize(shorter side) + CenterCrop, 1 = squash.  bit 1 (set by
                                   them too): the table blob carries the integer matrix-core form's tables and wise_preproc_u8
                                   uses that kernel; a caller may clear it (dot-product kernel) or set bit 2 with it (four waves per
                                   tile instead of one).  The three kernels return the same bytes. */
    uint64_t table_bytes;       /* size of the tap-table blob */
} wise_preproc_plan;
int wise_preproc_plan_init(int H, int W, int S, wise_preproc_plan* plan);
/* the same for open_clip's resize_mode 'squash' (the SigLIP models' preprocess_cfg): Resize((S, S), BICUBIC) without
 * regard to the aspect ratio, no crop — new_w = new_h = S, left = top = 0; same tables, same kernel */
int wise_preproc_plan_init_squash(int H, int W, int S, wise_preproc_plan* plan);
int wise_preproc_tables(const wise_preproc_plan* plan, void* host_tables);
/* frames uint8 [n,3,H,W] (device) -> out uint8 [n,3,S,S] (device, 4-byte aligned). */
int wise_preproc_u8(const wise_preproc_plan* plan, const void* dev_tables, const uint8_t* frames, int n,
                    uint8_t* out, void* stream);
/* Pillow's tap table of one axis (first input index, count, 22-bit fixed-point coefficients [out][ksize]);
 * host-only, exported so that the tables can be pinned against the oracle without a GPU. */
int wise_preproc_taps(int in_size, int out_size, int* ksize, int* first, int* count, int* coef,
                      int coef_capacity);

/* Building blocks, exported so the parity tests can pin each kernel separately. */
/* C[M,N] = epilogue(A[M,K] bf16 @ Wt[N,K]^T bf16 + bias[N]) ; M%128==0 rows must be readable
 * (callers pad), N%4==0, K%32==0.
 * mode: 0 -> out_bf16 = acc+bias ; 1 -> out_bf16 = quickgelu(acc+bias) ; 2 -> out_bf16 = gelu(acc+bias)
 *       3 -> resid_f32 += acc+bias (in place, fp32 residual stream) ; 4 -> out_f32 = acc+bias
 *       5 -> out_bf16 = gelu_tanh(acc+bias) ; 6 -> out_bf16 = relu(acc+bias) */
int wise_gemm_bf16(const uint16_t* A, const uint16_t* Wt, const float* bias, int M, int N, int K,
                   int mode, void* out, void* stream);
/* (ABI 5) The two GEMMs of wise_vit_config.ln_fold = 1: a LayerNorm between a residual GEMM and the next linear layer is
 * carried by the GEMMs themselves (open_clip's ln_1 / ln_2 as reached from src/feature/mlfoundation_openclip.py:99).
 *   wise_gemm_fold_resid: x += A[M,K] @ Wt[N,K]^T + bias on a residual stream kept as TWO bf16 arrays, x = hi + lo
 *     (hi = bf16(x), lo = bf16(x - hi), lo = hi + lo_off elements, lo_off >= M*N: 16 significand bits in the 4 bytes per
 *     element an fp32 stream takes — and hi is the next GEMM's operand as it stands); stats = one region of
 *     wise_gemm_fold_stats_bytes(M, N) bytes whose first M floats become rstd[r] = 1 / sqrt(var(x[r,:]) + eps); behind them
 *     wise_gemm_fold_counters_bytes(M) bytes of arrival counters (at byte offset wise_gemm_fold_counters_offset(M)) that must
 *     be ZERO on entry and are zero again on exit, then scratch (partial sums per 64 columns; per 32 with group32 != 0, which
 *     widths that are multiples of 192 but not of 128 need).  The statistics are reduced in one fixed tree, so a row's rstd
 *     does not depend on M or on the tile chosen (for one value of group32).
 *   wise_gemm_fold_bf16: out[M,N] bf16 = act(rstd[row] * (A @ Wt^T) + bias[col]), mode 0 / 1 / 2 / 5 as wise_gemm_bf16; with
 *     A = h, Wt = gamma-scaled row-centred weights and bias = b + W beta this is act(Linear(LayerNorm(x))).
 * M % 128 == 0, N % 128 == 0 (or N % 192 == 0 with group32), K % 64 == 0, K >= 192.  group32: bit 0 = statistics per 32
 * columns; bit 1 = the rows START the stream (x = A @ Wt^T + bias: nothing is read from hi / lo). */
size_t wise_gemm_fold_stats_bytes(int M, int N);
size_t wise_gemm_fold_counters_offset(int M);
size_t wise_gemm_fold_counters_bytes(int M);
int wise_gemm_fold_bf16(const uint16_t* A, const uint16_t* Wt, const float* bias, const float* rstd, int M, int N, int K,
                        int mode, uint16_t* out, void* stream);
int wise_gemm_fold_resid(const uint16_t* A, const uint16_t* Wt, const float* bias, int M, int N, int K, uint16_t* hi,
                         int64_t lo_off, float* stats, float eps, int group32, void* stream);
/* (ABI 5) wise_attention_bf16 followed by wise_gemm_fold_resid (N = K = 64 H) as ONE kernel, for sequences of up to 64
 * tokens and H = 12: per frame b, rows b*T .. b*T+T-1 of the hi + lo stream become x + softmax(q k^T / 8) v @ Wt^T + bias and
 * rstd[row] = 1 / sqrt(var(x[row,:]) + eps) — bit for bit what the two calls produce (same MFMA order, same reduction tree),
 * without the attention output's round trip through HBM, the arrival counters or the scratch region.  qkv [B*T, 3*64*H]
 * as wise_attention_bf16 takes it; Wt [64H, 64H], bias [64H]; rows past B*T are not touched.  Stands behind
 * open_clip's ResidualAttentionBlock.attention + ls_1 + residual as reached from src/feature/mlfoundation_openclip.py:99. */
int wise_attention_oproj_fold(const uint16_t* qkv, int B, int T, int H, const uint16_t* Wt, const float* bias, uint16_t* hi,
                              int64_t lo_off, float* rstd, float eps, void* stream);
/* (ABI 5) x[M,C] fp32 += fc2(GELU(fc1(h))) — erf GELU, h [M,C] bf16 (the LayerNorm'd rows), fc1: C -> 4C, fc2: 4C -> C — as ONE
 * kernel: the 4C-wide hidden activations stay in registers (rounded to bf16 where the two-GEMM form stores them).  C = 384
 * with M % 128 == 0, or C = 192 with M % 256 == 0: the MLP of a Swin block of HTSAT's stages 3 and 2 (msclap HTSAT
 * SwinTransformerBlock.mlp as reached from src/feature/microsoft_clap.py:49-50).  b1 [4C], b2 [C] fp32.  ws = both weight
 * matrices as ONE bf16 stream of 8 C^2 elements in the order the kernel consumes them: for every step s of 32 hidden units
 * (s < C/8) first the 2 * C/32 fc1 fragments (j = 0, 1; ks < C/32) and then the C/16 fc2 fragments (jn < C/16), a fragment
 * being 64 lanes x 8 elements with lane = 16 g + l:
 *   fc1 fragment (j, ks):  W1[32 s + 16 j + l][32 ks + 8 g + e],                        e < 8
 *   fc2 fragment (jn):     W2[16 jn + l][32 s + 4 g + e] for e < 4,  W2[16 jn + l][32 s + 16 + 4 g + (e - 4)] for e >= 4
 * (wise_amd/feature/htsat.py:mlp_stream_weights builds it). */
int wise_mlp_stream(const uint16_t* h, const uint16_t* ws, const float* b1, const float* b2, float* x, int M, int C,
                    void* stream);
/* the same with h = LayerNorm(x; lnw, lnb, eps) computed inside the kernel from the fp32 rows (norm2 of the block: two-pass
 * statistics in registers) — no LayerNorm launch and no h array; what wise_htsat_forward2 flags bit 1 runs. */
int wise_mlp_stream_ln(const float* lnw, const float* lnb, float eps, const uint16_t* ws, const float* b1, const float* b2,
                       float* x, int M, int C, void* stream);
/* (ABI 5) norm1 + QKV projection + window attention of a Swin block of HTSAT's stages 2 / 3 (C = 192 / 384: 8 / 16 heads of 24,
 * windows of 8 x 8 tokens on an H x H grid, cyclic shift 0 or 4) as ONE kernel: o [B*H*H, C] bf16 (original token order) =
 * softmax(q k^T / sqrt(24) + relb[head] (+ the shift mask)) v with q | k | v = LayerNorm(x; lnw, lnb, eps) W_qkv^T + b — what
 * wise_layernorm_f32_bf16 + wise_gemm_bf16 + the tower's window-attention kernel compute, without the normalised rows and the
 * qkv rows ever reaching HBM (msclap HTSAT WindowAttention as reached from src/feature/microsoft_clap.py:49-50).
 * x [B*H*H, C] fp32; relb [heads][64][64] fp32 (the expanded relative-position bias); B * (H/8)^2 even.
 * ws = W_qkv [3C, C] as a stream of 3 * C/48 steps, step s = 3 p + t (p: pair of heads, t: 0 q, 1 k, 2 v) holding weight rows
 * t*C + 48 p .. + 47 as 3 * C/32 fragments (j < 3, ks < C/32) of [lane = 16 g + l][8]: W[t*C + 48 p + 16 j + l][32 ks + 8 g + e];
 * bq = the qkv bias in the same step order, 48 floats per step (wise_amd/feature/htsat.py:swin_qkv_stream builds both). */
int wise_swin_qkv_attn(const float* x, const float* lnw, const float* lnb, float eps, const uint16_t* ws, const float* bq,
                       const float* relb, uint16_t* o, int B, int H, int C, int shift, void* stream);
/* out[ceil256(B*T*F), cout] bf16 = relu(conv3x3(x [B,T,F,cin] bf16, position-major ("NHWC"), stride 1, zero padding 1)
 * + bias[cout]); with pool != 0 its 2x2 average pooling (floor) instead, out [B*(T/2)*(F/2), cout], computed in the same
 * kernel (the unpooled tensor is never written).  wt [cout, 9*cin] bf16 with k = (kh*3 + kw)*cin + c (BatchNorm folded
 * by the caller); cin, cout multiples of 64; zeros = at least 16 bytes of zeros on the device (what every out-of-image
 * tap reads).  The implicit GEMM behind the ConvBlocks of wise_cnn14_forward
 * (torch: F.avg_pool2d(F.relu(bn(F.conv2d(x, w, padding=1))), 2)). */
int wise_conv3x3_relu_bf16(const uint16_t* x, const uint16_t* wt, const float* bias, const uint16_t* zeros, int batch,
                           int T, int F, int cin, int cout, int pool, uint16_t* out, void* stream);
/* LayerNorm fused into the GEMM's A operand: out_bf16[M,N] = epi( LN(x_f32[M,K]; lnw, lnb, eps) @ Wt[N,K]^T + bias ),
 * for K in {96, 192} (HTSAT stages 1-2), N % 8 == 0, M % 128 == 0, bf16 output modes (0, 1, 2, 5). */
int wise_gemm_ln_bf16(const float* x, const float* lnw, const float* lnb, const uint16_t* Wt, const float* bias,
                      int M, int N, int K, float eps, int mode, uint16_t* out, void* stream);
/* The MLP of a C = 96 Swin block in one kernel (HTSAT stage 1): x_f32[M,96] += fc2(gelu(fc1(LN(x; lnw, lnb, eps)))),
 * W1 [384,96], b1 [384], W2 [96,384], b2 [96]; M % 128 == 0.  The 384-wide hidden layer never reaches HBM. */
int wise_mlp96_fused(float* x, const float* lnw, const float* lnb, const uint16_t* W1, const float* b1,
                     const uint16_t* W2, const float* b2, int M, float eps, void* stream);
/* y_bf16[r,:] = (x[r,:]-mean)/sqrt(var+eps)*w+b over W for r < rows. */
int wise_layernorm_f32_bf16(const float* x, const float* w, const float* b, int rows, int W,
                            float eps, uint16_t* y, void* stream);
/* qkv [B*T, 3*H*64] bf16 (q|k|v packed like in_proj) -> o [B*T, H*64] bf16 ; softmax(QK^T/8)V */
int wise_attention_bf16(const uint16_t* qkv, int B, int T, int H, uint16_t* o, void* stream);
/* the same at head dim dh = 64 or 80 (ViT-H/14: width 1280 over 16 heads): qkv [B*T, 3*H*dh], softmax(QK^T/sqrt(dh))V */
int wise_attention_dh_bf16(const uint16_t* qkv, int B, int T, int H, int dh, uint16_t* o, void* stream);
/* head dim 64, right-padded sequences: sequence b has lens[b] (device int32 [B], 1..T) keys; keys past it are masked for
 * every query of that sequence (the BERT-family text towers, wise_xlmr_forward).  lens[b] outside 1..T is clamped into it:
 * 0 (or less) counts as one key, more than T as T.  Every query row is written, rows past lens[b] included: they attend
 * the same lens[b] keys (tests/test_gpu_attention_exact.py pins both). */
int wise_attention_lens_bf16(const uint16_t* qkv, int B, int T, int H, const int32_t* lens, uint16_t* o, void* stream);
/* head dim 64 with the causal mask of the text tower: query t attends keys <= t */
int wise_attention_causal_bf16(const uint16_t* qkv, int B, int T, int H, uint16_t* o, void* stream);

/* (ABI 5) search_grouped: the k best GROUPS of rows (videos, shots, files), one hit per group.  Not in the reference, which groups
 * the top `end` <= 1000 rows by media_id AFTER the search (api/routes.py:582-596) and so shows a dozen results when a thousand best
 * frames come from a dozen files.  Every stored row belongs to one group; over a query's CANDIDATE rows — every row of an exhaustive
 * index, the rows of the probed lists of an inverted-file index, under a selector only the selected ones — a group's representative
 * is its candidate row with the best score, ties to the lower row position (the row of the payload; the position in list order),
 * and the answer is the k groups whose representatives are best, in the order of the representatives' (score, position) keys: the
 * tie rule of the scans.  Three stages, all on the device, no global atomics, the same bytes on every run:
 *   1  a *_group_scores call writes, per (query, candidate row), ord[q][row] = the 32-bit ordered image of the key score (the
 *      score; the negated squared distance for the L2 types): u = the float's bits, u ^ 0x80000000 where u >= 0, ~u where u < 0 — the
 *      upper half of the scans' 64-bit keys.  The score is, bit for bit, what the type's exact top-k scan gives that (query, row).
 *      0 = no candidate.  ord [nq][N] uint32.  keep: a selector's bitmap over the positions (wise_sel_bitmap), or null.  The
 *      arguments before `keep` are those of the type's range count entry point without radius, counts and workspace; the calls
 *      over inverted lists clear ord first (the rows of the lists a query does not probe read 0), the exhaustive ones write every
 *      row.  wise_ipsq8_group_scores takes W and q0 of wise_sq_query, as the wise_ivfsq_* entry points do.
 *   2  wise_group_best: best[q][g] = the maximum over the rows r of group g of (ord[q][r] << 32) | (0xFFFFFFFF - r), 0 for a
 *      group without a candidate.  group_rows [N] uint32: the row positions sorted by (group, position); group_off [G + 1]: group g
 *      owns group_rows[group_off[g] .. group_off[g + 1]), group_off[0] = 0, group_off[G] = N, ascending.  best [nq][G] uint64.
 *   3  wise_group_topk: the k largest keys of each query -> outD / outI / outG [nq][k]: the representative's score (flip != 0: the
 *      key score negated back into a distance), its external id (ids[row], or id_base + row where ids is null) and its group's
 *      key group_keys[gid[row]] (gid [N] int32: the group of every row, group_keys [G] int64).  Slots no group fills hold
 *      (-3.4028235e38, -1, -1); flip != 0: (+3.4028235e38, -1, -1).  workspace: the merge parts.
 * Limits: N < 2^32 - 1, 0 <= G <= min(N, 2^31 - 1) (gid is int32), 1 <= nq <= 65535, 1 <= k <= 2048, d as each type's scan takes it; anything else returns
 * WISE_E_INVALID and leaves the outputs untouched.  wise_group_workspace_bytes: ord, best and the merge parts of nq queries in
 * one allocation, each region aligned to 256 bytes, in this order — 4 N + 8 G bytes a query plus the parts —; 0 for an
 * unsupported shape.  wise_group_topk itself needs only the last region. */
size_t wise_group_workspace_bytes(int64_t N, int64_t G, int nq, int k);
int wise_ip_group_scores_f32(const float* X, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord, void* stream);
int wise_ipsq16_group_scores(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord,
                             void* stream);
int wise_ipsq8_group_scores(const uint8_t* codes, int64_t N, int d, const float* W, const float* q0, int nq, const uint32_t* keep,
                            uint32_t* ord, void* stream);
int wise_l2_group_scores_f32(const float* X, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord, void* stream);
int wise_l2sq16_group_scores(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord,
                             void* stream);
int wise_ivf_group_scores_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                              const int64_t* probes, int nprobe, const uint32_t* keep, uint32_t* ord, void* stream);
int wise_ivfsq_group_scores(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const float* W, const float* q0,
                            int nq, const int64_t* probes, const float* bias, int nprobe, const uint32_t* keep, uint32_t* ord,
                            void* stream);
int wise_ivfsq16_group_scores(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                              const int64_t* probes, const float* bias, int nprobe, const uint32_t* keep, uint32_t* ord, void* stream);
int wise_ivfl2_group_scores(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                            const int64_t* probes, int nprobe, const uint32_t* keep, uint32_t* ord, void* stream);
int wise_group_best(const uint32_t* ord, int64_t N, int nq, const int64_t* group_off, const uint32_t* group_rows, int64_t G,
                    uint64_t* best, void* stream);
int wise_group_topk(const uint64_t* best, int64_t G, int nq, int k, const int32_t* gid, int64_t N, const int64_t* group_keys,
                    const int64_t* ids, int64_t id_base, int flip, float* outD, int64_t* outI, int64_t* outG, void* workspace,
                    size_t workspace_bytes, void* stream);

/* (ABI 5) Selectors over GROUPS and trees of selectors (csrc/sel_tree.hip; wise_amd/index/selector.py: IDSelectorGroups,
 * IDSelectorBitmap, IDSelectorAnd / Or / XOr, IDSelectorNot over anything).  Every entry writes or combines bitmaps of the layout and
 * with the guarantees of wise_sel_bitmap: (N + 31) / 32 uint32 words, ALL written, bit (p & 31) of word p >> 5, and the bits past N
 * are zero, also when inverted — what the *_scan_sel, *_topk_pos (through wise_sel_positions), *_range_count, *_group_scores and
 * wise_compact_* entry points take.  One lane per row, a wave's 64 answers are one ballot written by one lane as two words; no
 * atomics, the same bits on every run; nothing allocates or reads back, so every call can be captured into a graph.
 * Limits: 0 <= N < 2^32 - 1 (N = 0: nothing is launched and no pointer is looked at), 0 <= G <= 2^31 - 1 (gid is int32), n_sel >= 0,
 * n_bytes >= 0, op in 0 .. 4.  Anything else — also a null pointer where rows exist (gid, bitmap, a, out; group_keys where G > 0;
 * sel_keys where n_sel > 0; bits where n_bytes > 0; b where op != 4), or, where N > 0, a workspace that is null or shorter than
 * wise_sel_groups_workspace_bytes(G) — is WISE_E_INVALID with a wise_last_error text, and nothing is written.  The checks need no
 * device.
 *   wise_sel_bitmap_groups: bit p = 1 iff 0 <= gid[p] < G and group_keys[gid[p]] occurs in sel_keys.  gid [N] int32 and group_keys
 *     [G] int64 ascending are the group tables of set_groups (wise_group_topk reads the same two); sel_keys [n_sel] int64 sorted
 *     ascending without duplicates.  n_sel = 0 selects nothing, and so does a key no group carries; invert != 0 complements the
 *     answer within the index; G = 0 is legal (no row has a group: all zero, or all N bits set when inverted).  Two launches: a
 *     MARK pass, one lane per group, a binary search of its key in sel_keys, G bits into the workspace; a ROW pass, one lane per
 *     row, which reads gid[p] and tests that group's mark bit.  The device reads 4 N bytes and writes N / 8.
 *     wise_sel_groups_workspace_bytes(G): the mark bits, a multiple of 256 bytes and never 0 for a legal G; 0 for G out of range.
 *   wise_sel_bitmap_idbits: faiss's IDSelectorBitmap.  The external id i of row p is ids[p], or id_base + p with ids == NULL; i is
 *     selected iff i >= 0, (i >> 3) < n_bytes and (bits[i >> 3] >> (i & 7)) & 1.  n_bytes = 0 selects nothing; invert as above.
 *   wise_sel_combine: word by word over two bitmaps of N positions, op 0: a AND b, 1: a OR b, 2: a XOR b, 3: a AND NOT b, 4: NOT a
 *     (b is ignored and may be NULL).  out may be a or b (any other overlap is undefined).  The tail bits of out are zero for
 *     every op, whatever the tails of a and b hold.  Words go four at a time where a, b and out are 16-byte aligned. */
size_t wise_sel_groups_workspace_bytes(int64_t G);
int wise_sel_bitmap_groups(const int32_t* gid, int64_t N, const int64_t* group_keys, int64_t G, const int64_t* sel_keys, int64_t n_sel,
                           int invert, uint32_t* bitmap, void* workspace, size_t workspace_bytes, void* stream);
int wise_sel_bitmap_idbits(const int64_t* ids, int64_t id_base, int64_t N, const uint8_t* bits, int64_t n_bytes, int invert,
                           uint32_t* bitmap, void* stream);
int wise_sel_combine(const uint32_t* a, const uint32_t* b, int64_t N, int op, uint32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WISE_HIP_H */
