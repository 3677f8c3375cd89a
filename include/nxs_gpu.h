/*
 * nxs_gpu.h -- C-ABI of the HIP (gfx950 / MI355X) side of the query path.
 *
 * This is the thin shim the C11 host code (nxsearch_amd/csrc/nxs_*.c) calls;
 * no HIP or C++ types cross it: plain pointers, sizes and PODs.  Each entry
 * names the reference seam it replaces.
 *
 *   nxsgpu_index_create  <- idx_dtmap_sync + dtmap_build_tdmap
 *                           (src/index/dtmap.c:386-544): builds the reverse
 *                           index (here: CSR posting arrays in HBM, transposed
 *                           from the nxsdtmap image on the device) and the
 *                           BK-tree image (src/index/idxterm.c:157-187).
 *   nxsgpu_search        <- run_query_logic + get_expr_bitmap
 *                           (src/query/search.c:118-278) with the
 *                           ranking_func_t seam (src/core/nxs_impl.h:52-53;
 *                           src/algo/ranking.c:41-176) and
 *                           nxs_resp_addresult/nxs_resp_build
 *                           (src/core/results.c:128-220; src/algo/heap.c).
 *   nxsgpu_fuzzy         <- idxterm_fuzzysearch (src/index/idxterm.c:210-249)
 *                           = bktree_search (src/algo/bktree.c:219-275) with
 *                           the bktree_distfunc_t seam bound to levdist
 *                           (src/algo/levdist.c:67-150).
 *   nxsgpu_suggest       (new: no seam in the reference) every term near a
 *                           token, ranked -- the same screen and distance.
 *   nxsgpu_complete      (new: no seam in the reference) every live term that
 *                           begins with a prefix, ranked by df -- a range of
 *                           the terms' byte order.
 *   nxsgpu_wildcard      (new: no seam in the reference) every live term that
 *                           matches a `*` / `?` pattern, ranked by df -- a scan
 *                           of the range its literal head selects.
 */
#ifndef NXS_GPU_H
#define NXS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define	NXSGPU_MAX_TOKENS	32	/* tokens per query on the device path */
#define	NXSGPU_MAX_PROG		256	/* postfix program bytes */
#define	NXSGPU_FAST_K		64	/* limit up to which the heap lives across the lanes of a wavefront */
#define	NXSGPU_BIG_K		8000	/* limit up to which the candidate filter applies (heap in LDS);
					 * beyond it: the exact two-pass path */

/* ranking_algo_t (reference src/index/index.h:30-34) */
#define	NXSGPU_TF_IDF		0
#define	NXSGPU_BM25		1

/* postfix opcodes: 0..31 push presence bit of token i */
#define	NXSGPU_OP_EMPTY		0x40	/* push the empty set (search.c:140) */
#define	NXSGPU_OP_AND		0x80	/* roaring64_bitmap_and_inplace    */
#define	NXSGPU_OP_OR		0x81	/* roaring64_bitmap_or_inplace     */
#define	NXSGPU_OP_ANDNOT	0x82	/* roaring64_bitmap_andnot_inplace */

typedef struct nxsgpu_index nxsgpu_index_t;

/*
 * One flattened BK-tree node (BFS numbering: index = BFS rank, the children of
 * a node are contiguous and in ascending slot order -- bktree.c:54-58,79-98).
 */
typedef struct {
	uint64_t	bitmap;		/* child slots (distance 1..63)       */
	uint32_t	first_child;	/* BFS index of the lowest-slot child */
	uint32_t	term_id;
	uint32_t	str_off;	/* term bytes in the byte pool        */
	uint16_t	str_len;
	uint16_t	flags;		/* bit 0: on-disk total count > 0     */
	uint8_t		inl[8];		/* first 8 term bytes (zero padded)   */
} nxsgpu_bknode_t;

typedef struct {
	/* nxsdtmap image (host memory) and the live doc blocks in it */
	const uint8_t *	dtmap_img;
	uint64_t	dtmap_len;
	const uint64_t *blk_off;	/* [n_docs] block offsets, ascending doc id */
	const uint64_t *doc_ids;	/* [n_docs] ascending                       */
	const uint64_t *pair_base;	/* [n_docs+1] prefix sum of per-doc n       */
	uint64_t	n_docs;
	/* term-id space of nxsterms: ids 1..n_terms; term_ok[id]=1 if live */
	uint32_t	n_terms;
	const uint8_t *	term_ok;	/* [n_terms+1] */
	/* header counters (dtmap.c:660-677) */
	uint32_t	hdr_doc_count;
	uint64_t	hdr_token_count;
	/* flattened BK-tree */
	const nxsgpu_bknode_t *bk_nodes;
	uint32_t	n_bk;
	uint32_t	bk_depth;	/* number of BFS levels */
	const uint8_t *	bk_bytes;
	uint64_t	bk_bytes_len;
	/* the index's ranking function (params.db "algo"): its impacts are built with
	 * the index, the other function's on the first search that asks for it; -1: both */
	int		default_algo;
} nxsgpu_index_src_t;

/* one resolved query */
typedef struct nxsgpu_query {
	uint32_t	n_tokens;			/* token-list order */
	uint32_t	term_id[NXSGPU_MAX_TOKENS];
	uint32_t	prog_len;
	uint8_t		prog[NXSGPU_MAX_PROG];
	uint32_t	truth[8];	/* 256-bit truth table, valid if n_tokens <= 8 */
} nxsgpu_query_t;

typedef struct {
	uint32_t	n_queries;
	uint32_t *	counts;		/* [n]   results per query          */
	uint64_t *	offsets;	/* [n+1] into doc_ids / scores      */
	uint64_t *	doc_ids;
	float *		scores;
	/* work counters of the call */
	uint64_t	postings;	/* postings streamed                */
	uint64_t	candidates;	/* (doc,score) handed to the replay */
	uint32_t	exact_requeries;/* queries re-run through the two-pass path */
} nxsgpu_results_t;

#define	NXSGPU_PROF_CLS	16
typedef struct {
	uint64_t	launches;	/* launches of the dominant scan kernel */
	double		scan_ms;	/* summed HIP-event time of those      */
	double		replay_ms;
	double		fuzzy_ms;
	uint64_t	postings;	/* summed algorithmic postings         */
	uint64_t	fuzzy_visits;	/* Levenshtein distance evaluations    */
	uint64_t	fuzzy_pairs;	/* (token, node) pairs dequeued        */
	uint64_t	fuzzy_level[40];/* ... per BFS level                   */
	/* match-first search, per kernel (HIP events on the fuzzy stream) */
	double		fuzzy_filter_ms;/* k_bk_peq + k_bk_seed + k_fz_filter   */
	double		fuzzy_dist_ms;	/* k_fz_dist                           */
	double		fuzzy_chain_ms;	/* k_fz_chain + k_bk_finish            */
	uint64_t	fuzzy_checked;	/* (token, term) pairs k_fz_filter compared */
	/*
	 * Per query CLASS (= one scan launch per batch): HIP events recorded on the stream
	 * the class's kernels are launched on, around them.  cls_key = kind << 8 | shape << 4
	 * bits | token bucket (nxs_gpu_int.h: cls_kind_t, cls_shape_t; nxs_gpu_plan.hip: classify_query); kind 1
	 * k_scan1 / k_scan8, 3 k_scanr, 4 k_scanm, 5 k_cold + k_scanm<.., DROP>, 6 k_scanb, 7 k_scanq, 8 k_scans,
	 * 9 k_cold + k_scans<.., DROP>, 0 k_scan.  Bit 7: a launch of the class's top doc ranges, sent ahead.
	 */
	uint32_t	n_cls;
	uint32_t	cls_key[NXSGPU_PROF_CLS];
	uint64_t	cls_launches[NXSGPU_PROF_CLS];
	double		cls_ms[NXSGPU_PROF_CLS];
	uint64_t	cls_postings[NXSGPU_PROF_CLS];	/* algorithmic postings of the class's queries */
	uint64_t	cls_queries[NXSGPU_PROF_CLS];
} nxsgpu_profile_t;

int		nxsgpu_device_count(void);
const char *	nxsgpu_last_error(void);

nxsgpu_index_t *nxsgpu_index_create(int device, const nxsgpu_index_src_t *);
void		nxsgpu_index_destroy(nxsgpu_index_t *);

/*
 * N1 -- incremental refresh: what idx_terms_sync / idx_dtmap_sync consumed since
 * the last snapshot (src/index/terms.c:320-414, src/index/dtmap.c:440-544),
 * validated by the host: appended docs carry ids above every loaded one (they
 * take the highest ordinals) and name known terms only.
 */
typedef struct {
	uint32_t	n_terms;	/* new last term id (>= the old one) */
	const uint8_t *	term_ok;	/* [n_terms+1] */
	const uint8_t *	dtmap_img;	/* the mapped nxsdtmap image */
	uint64_t	dtmap_len;
	const uint64_t *blk_off;	/* [n_new] appended doc blocks, ascending doc id */
	const uint64_t *doc_ids;	/* [n_new] */
	const uint64_t *pair_base;	/* [n_new+1] */
	uint64_t	n_new;
	const uint32_t *dead_term;	/* (term, ordinal) of every posting of a removed doc */
	const uint32_t *dead_ord;
	uint64_t	n_dead_pairs;
	uint32_t	hdr_doc_count;	/* header counters now (dtmap.c:660-677) */
	uint64_t	hdr_token_count;
	/* doc shards (N4): merge only; the impacts wait for the collection-wide df
	 * of the new term count (nxsgpu_index_set_global_df) and are computed once */
	int		defer_impacts;
} nxsgpu_index_delta_t;

/* merge the delta into the device CSR and recompute every impact (unless
 * deferred); 0 / -1 (the index is unchanged on failure unless the error says
 * otherwise) */
int		nxsgpu_index_apply(nxsgpu_index_t *, const nxsgpu_index_delta_t *);
/* replace the BK-tree image (after terms were inserted on the host) */
int		nxsgpu_index_set_bk(nxsgpu_index_t *, const nxsgpu_bknode_t *nodes, uint32_t n,
		    uint32_t depth, const uint8_t *bytes, uint64_t bytes_len);

/*
 * N4 -- doc-sharded mode (collections beyond one GPU's HBM): every shard holds
 * the postings of a contiguous range of docs (ascending doc id) but scores with
 * COLLECTION-WIDE statistics: N and the token count come from the file header,
 * df is handed in (sum of the shards' nxsgpu_index_df) and all impacts are
 * recomputed.  A query then runs on every shard, each returns the exact
 * sequence of candidates its local heap accepted, and the sequences -- highest
 * shard first -- are replayed through the reference's heap once more
 * (nxsgpu_merge_candidates): identical top-k, ties included.
 */
int		nxsgpu_index_set_global_df(nxsgpu_index_t *, const uint32_t *df, uint32_t n_terms);
/* full impact passes since the index was built (each recomputes every impact) */
uint64_t	nxsgpu_index_impact_passes(const nxsgpu_index_t *);
/* ids/scores [n_queries][cap], counts [n_queries] (host); counts[q] > cap = overflow */
int		nxsgpu_search_candidates(nxsgpu_index_t *, int algo, uint64_t limit,
		    const nxsgpu_query_t *queries, uint32_t n_queries, uint32_t cap,
		    uint64_t *ids, float *scores, uint32_t *counts);
/* ids/scores [nq][n_shards][cap], counts [nq][n_shards], shard 0 = lowest docs;
 * out_* [nq][limit] / [nq]; limit <= NXSGPU_FAST_K */
int		nxsgpu_merge_candidates(int device, uint32_t limit, uint32_t nq, uint32_t n_shards,
		    uint32_t cap, const uint64_t *ids, const float *scores, const uint32_t *counts,
		    uint64_t *out_ids, float *out_scores, uint32_t *out_counts);

/* document frequency per term id [n_terms+1] (host buffer) */
int		nxsgpu_index_df(nxsgpu_index_t *, uint32_t *df);
uint64_t	nxsgpu_index_postings(const nxsgpu_index_t *);
uint64_t	nxsgpu_index_docs(const nxsgpu_index_t *);
/* first live doc (file order) whose block names an unknown term, or ~0 */
uint64_t	nxsgpu_index_first_bad_doc(const nxsgpu_index_t *);

/*
 * Threading: an nxsgpu_index_t belongs to ONE host thread at a time, like the
 * reference's nxs_t (docs/c-api.md:5-8).  A blocking nxsgpu_search() while batches
 * are in flight runs on stream and event sets of its own (it swaps them into the
 * index for the call): another thread calling into the same index meanwhile would
 * enqueue on the wrong streams.
 */
int		nxsgpu_search(nxsgpu_index_t *, int algo, uint64_t limit,
		    const nxsgpu_query_t *queries, uint32_t n_queries,
		    nxsgpu_results_t *res);
void		nxsgpu_results_free(nxsgpu_results_t *);

/*
 * Queries that do not fit nxsgpu_query_t (more than NXSGPU_MAX_TOKENS live
 * tokens, a program of more than NXSGPU_MAX_PROG items, or an evaluation
 * stack deeper than 64): run_query_logic (search.c:210-278) has no such
 * bounds.  Variable-size plan, generic kernel, always the exact two-pass path.
 */
#define	NXSGPU_WIDE_MAX_TOKENS	1024
#define	NXSGPU_WOP_AND		0xfff0u
#define	NXSGPU_WOP_OR		0xfff1u
#define	NXSGPU_WOP_ANDNOT	0xfff2u
#define	NXSGPU_WOP_EMPTY	0xffffu	/* push the empty set (search.c:140) */

typedef struct {
	uint32_t	n_tokens;	/* token-list order */
	const uint32_t *term_id;
	uint32_t	prog_len;
	const uint16_t *prog;		/* postfix: < 0x8000 pushes token i, else NXSGPU_WOP_* */
} nxsgpu_wide_query_t;

int		nxsgpu_search_wide(nxsgpu_index_t *, int algo, uint64_t limit,
		    const nxsgpu_wide_query_t *queries, uint32_t n_queries,
		    nxsgpu_results_t *res);

/*
 * Device-resident variant for multi-GPU gathers: limit <= NXSGPU_FAST_K,
 * outputs are DEVICE pointers laid out [n_queries][limit] / [n_queries],
 * left on the device (no host copy).  Returns 0, or 1 if some query needs the
 * exact two-pass path (then call nxsgpu_search for it), -1 on error.
 */
int		nxsgpu_search_dev(nxsgpu_index_t *, int algo, uint32_t limit,
		    const nxsgpu_query_t *queries, uint32_t n_queries,
		    uint64_t *d_doc_ids, float *d_scores, uint32_t *d_counts);

/*
 * The same, split for pipelining: _begin() plans the batch on the host, sends
 * the plans up and queues the kernels, then returns; _end() waits for the
 * OLDEST batch in flight and returns its status (0 / 1 / -1 as above).  Up to
 * NXSGPU_INFLIGHT batches may be in flight, so the host prepares batch i+1 while
 * batch i runs (two in flight hide the host side of a top-10 batch; limits in the
 * hundreds end in a heap replay of milliseconds -- one wavefront per query, the
 * chip nearly idle -- and take three or four to fill the GPU); each needs its own
 * output buffers until its _end().  nxsgpu_search() and nxsgpu_search_dev()
 * refuse to run while a batch is in flight.
 */
#define	NXSGPU_INFLIGHT	4
int		nxsgpu_search_dev_begin(nxsgpu_index_t *, int algo, uint32_t limit,
		    const nxsgpu_query_t *queries, uint32_t n_queries,
		    uint64_t *d_doc_ids, float *d_scores, uint32_t *d_counts);
int		nxsgpu_search_dev_end(nxsgpu_index_t *);

int		nxsgpu_fuzzy(nxsgpu_index_t *, const uint8_t *tok_bytes,
		    const uint32_t *tok_off, uint32_t n_tokens,
		    uint32_t *term_ids, uint64_t *visited);
/*
 * The same search split in two (no visit counts): _begin queues the device pass on the fuzzy stream and
 * returns a slot (>= 0; -1 error; -2 all NXSGPU_FZ_SLOTS slots taken), _end -- with the slot and the same
 * tokens -- waits and delivers.  The host's planning of the NEXT batch and the scans of the batches in
 * flight run meanwhile (nxs_batch.c: a batch with misses is finished by the next
 * nxs_index_search_batch_begin).  Passes run, and are to be ended, in the order they were begun;
 * nxsgpu_fuzzy() refuses to run while one is in flight.
 */
#define	NXSGPU_FZ_SLOTS	2
int		nxsgpu_fuzzy_begin(nxsgpu_index_t *, const uint8_t *tok_bytes,
		    const uint32_t *tok_off, uint32_t n_tokens);
int		nxsgpu_fuzzy_end(nxsgpu_index_t *, int slot, const uint8_t *tok_bytes,
		    const uint32_t *tok_off, uint32_t n_tokens, uint32_t *term_ids);

/*
 * ---- spelling suggestions ----------------------------------------------------------
 *
 * nxsgpu_suggest: for each of n_tokens raw tokens (bytes tok_off[i] .. tok_off[i + 1], already through the
 * index's filters) the ELIGIBLE terms -- a posting in a live doc (df > 0, what nxsgpu_index_df reports) and
 * byte-wise Levenshtein distance <= maxdist (1 or 2) -- in the order distance ascending, df descending, term
 * id ascending.  Rows of k (1..32) entries: term_ids / dist / df [n_tokens][k], counts[i] = min(k, matches[i])
 * entries of row i are valid, matches[i] is the exact number of eligible terms.  This is not the set the
 * BK walk of nxsgpu_fuzzy visits: terms below a slot-63 child count, terms whose docs are all removed do
 * not, and an exact hit comes first.
 *
 * The pass shares the match-first search's screen (k_fz_filter) over a candidate permutation of its own,
 * built by the first call and rebuilt after nxsgpu_index_apply / _set_bk / _set_global_df (a generation
 * counter: an index that is never asked builds, uploads and launches nothing).  It runs on a stream and
 * workspace of its own: allowed while batches and fuzzy passes (nxsgpu_fuzzy_begin) are in flight, takes
 * none of their slots.  A queue that overflows (NXS_GPU_FUZZY_CAND bounds the survivor queues) repeats the
 * pass with fewer tokens, down to one token with queues of 8 bytes x candidates: answers never change.
 * Tokens of more than 64 bytes, and every token under NXS_GPU_SUGGEST=host (the cross-check route), are
 * ranked on the host over a copy of the BK image.  0 / -1.
 *
 * nxsgpu_suggest_profile (nxsgpu_set_profiling): since the last reset -- out[0] device passes, out[1] their
 * HIP-event ms, out[2] k_bk_peq + k_fz_filter, out[3] k_sg_dist, out[4] k_sg_scan + k_sg_scatter, out[5]
 * k_sg_select, out[6] survivors of the screen, out[7] matches, out[8] tokens ranked on the host (counted
 * always), out[9] passes repeated after an overflow (counted always).
 */
#define	NXSGPU_SUGGEST_PROF	10
int		nxsgpu_suggest(nxsgpu_index_t *, const uint8_t *tok_bytes, const uint32_t *tok_off,
		    uint32_t n_tokens, uint32_t maxdist, uint32_t k,
		    uint32_t *term_ids, uint8_t *dist, uint32_t *df, uint32_t *counts, uint32_t *matches);
void		nxsgpu_suggest_profile(nxsgpu_index_t *, double out[NXSGPU_SUGGEST_PROF], int reset);

/*
 * ---- prefix completion --------------------------------------------------------------
 *
 * nxsgpu_complete: for each of n prefixes (bytes off[i] .. off[i + 1], already normalised) the ELIGIBLE terms
 * -- a posting in a live doc (df > 0, what nxsgpu_index_df reports) and the first len(p) bytes equal to p, the
 * term equal to p included -- in the order df descending, term id ascending.  Rows of k (1..32) entries:
 * term_ids / df [n][k], counts[i] = min(k, matches[i]) entries of row i are valid, matches[i] is the exact
 * number of eligible terms.  An empty prefix matches every live term.
 *
 * The live terms of every length are kept in byte-lexicographic order on the device (one stable radix sort
 * per 8-byte chunk, last chunk first), each with its (df, term id) beside it; a prefix is then two binary
 * searches (k_px_range: the range's length IS the match count) and a selection over the range
 * (k_px_select, one workgroup per prefix).  The order is built by the first call and rebuilt after
 * nxsgpu_index_apply / _set_bk / _set_global_df (a generation counter: an index that is never asked builds,
 * uploads and launches nothing).  The pass runs on a stream and workspace of its own: allowed while batches
 * and fuzzy passes are in flight, takes none of their slots; blocking.  Under NXS_GPU_COMPLETE=host (the
 * cross-check route) every prefix is ranked on the host over a copy of the BK image.  0 / -1.
 *
 * nxsgpu_complete_profile: since the last reset -- out[0] device passes, out[1] their HIP-event ms, out[2]
 * k_px_range, out[3] k_px_select (out[0..3] with nxsgpu_set_profiling only), out[4] wall ms of the last build
 * of the order (or of the host copy), out[5] entries in it, out[6] prefixes answered on the host, out[7]
 * builds of the order.
 */
#define	NXSGPU_COMPLETE_PROF	8
int		nxsgpu_complete(nxsgpu_index_t *, const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t k,
		    uint32_t *term_ids, uint32_t *df, uint32_t *counts, uint32_t *matches);	/* rows [n][k]; 0 / -1 */
void		nxsgpu_complete_profile(nxsgpu_index_t *, double out[NXSGPU_COMPLETE_PROF], int reset);

/*
 * ---- wildcard term matching ---------------------------------------------------------
 *
 * nxsgpu_wildcard: for each of n patterns (bytes off[i] .. off[i + 1], already normalised, at most 255 bytes:
 * `*` any run of bytes, `?` one byte, every other byte itself; csrc/nxs_wild.h) the ELIGIBLE terms -- a posting
 * in a live doc (df > 0) and the whole term matches the whole pattern -- in the order df descending, term id
 * ascending.  Rows of k (1..32) entries as nxsgpu_complete's: term_ids / df [n][k], counts[i] = min(k,
 * matches[i]), matches[i] the exact number of eligible terms, however large.
 *
 * The pass reads nxsgpu_complete's order of the live terms (built by whichever call comes first, rebuilt when
 * the generation has moved) and builds none of its own: the pattern's literal head selects a range of it by
 * the same two binary searches (all of it when the pattern begins with a metacharacter), k_wc_match scans
 * the range -- (part of a range, pattern) per workgroup, at most NXS_GPU_WILD_PARTS (default 64) parts, a
 * running top-k per workgroup in LDS, matches counted by ballot -- and k_wc_merge selects the k best of a
 * pattern's parts.  Device memory is n x parts x k keys, never a list of matches; a batch whose partial lists
 * would exceed 64 MiB is cut into chunks of patterns.  Stream, workspace and concurrency as nxsgpu_complete;
 * blocking.  Under NXS_GPU_WILDCARD=host (the cross-check route) every pattern is ranked on the host over a
 * copy of the BK image.  0 / -1.
 *
 * nxsgpu_wildcard_profile: since the last reset -- out[0] device passes (chunks), out[1] their HIP-event ms,
 * out[2] the range searches, out[3] k_wc_match, out[4] k_wc_merge (out[1..4] with nxsgpu_set_profiling only),
 * out[6] patterns answered on the host, out[8] patterns answered on the device; not reset: out[5] entries in
 * the order (or the host copy), out[7] builds of the order or of the host copy since the index was created
 * (nxsgpu_complete's builds included: the two calls share them, and each route builds its own once per
 * generation).
 */
#define	NXSGPU_WILDCARD_PROF	10
int		nxsgpu_wildcard(nxsgpu_index_t *, const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t k,
		    uint32_t *term_ids, uint32_t *df, uint32_t *counts, uint32_t *matches);	/* rows [n][k]; 0 / -1 */
void		nxsgpu_wildcard_profile(nxsgpu_index_t *, double out[NXSGPU_WILDCARD_PROF], int reset);

/*
 * ---- explanations -------------------------------------------------------------------
 *
 * nxsgpu_explain: for final results, what every token of the query's token list added to every returned doc.
 * run_query_logic (search.c:236-270) adds rank(term, doc) to a doc's score for every token, in list order,
 * whose term holds the doc (the expression only decides which docs are looked at; a term listed twice adds
 * twice), so the present cells of a row, added in f32 in ascending token order, are the doc's score bit for
 * bit.
 *
 * rows: for query q the results doc_ids[res_off[q] .. res_off[q+1]) x its n_tok[q] tokens
 * (term ids tok_ids[tok_off[q] ..]); out_tf / out_imp are [sum_q results(q) * n_tok(q)], row-major
 * (result, token); tf == 0 means absent (a posting's tf is >= 1); found[r] == 0: doc id r is not a
 * live doc of THIS index (doc shards) and its row is all absent.  (out_* and found are indexed from the
 * first result of the call, res_off[0].)  A term id outside the dictionary and a term without live
 * postings are absent everywhere.  0 / -1.
 *
 * The pass (k_explain: a lane per result, the token loop wave-uniform, nxs_explain.h's searches) reads the
 * index's arrays as they are at call time, on a stream and a grow-only workspace of its own: allowed while
 * batches and fuzzy passes are in flight, takes none of their slots; blocking.  It is cut into chunks of at
 * most NXS_GPU_EXPLAIN_ROWS cells (default 2 M: 36 MB of workspace at most).  An index that is never asked
 * allocates, uploads and launches nothing.  The ranking function's impacts must be materialised (they are
 * for any result that exists).
 *
 * nxsgpu_explain_profile: since the last reset -- out[0] passes (calls that reached the device), out[1]
 * HIP-event ms of k_explain (with nxsgpu_set_profiling only), out[2] cells, out[3] cells present, out[4]
 * chunks (kernel launches).
 */
#define	NXSGPU_EXPLAIN_PROF	8
int		nxsgpu_explain(nxsgpu_index_t *, int algo, uint32_t n_queries,
		    const uint32_t *tok_off, const uint32_t *tok_ids,
		    const uint64_t *res_off, const uint64_t *doc_ids,
		    uint32_t *out_tf, float *out_imp, uint8_t *found);
void		nxsgpu_explain_profile(nxsgpu_index_t *, double out[NXSGPU_EXPLAIN_PROF], int reset);

/*
 * ---- term vectors of docs -------------------------------------------------------------
 *
 * nxsgpu_doc_terms: for each of n doc ids the ELIGIBLE terms -- a posting in the doc, a live df (the length
 * of the term's list, what nxsgpu_index_df reports) >= mindf, and the float w = rank(term, doc) under `algo`
 * (what nxsgpu_explain reports for the pair: d_post[algo] at the posting's position; the REGULAR posting of a
 * TF-IDF dense term, never its outlier list) >= 0 -- in the order w descending as floats, term id ascending.
 * Rows of k (1..NXSGPU_DOCTERMS_MAX) entries: term_ids / w / tf / df [n][k], counts[i] = min(k, matches[i]),
 * matches[i] the exact number of eligible terms, however large; found[i] == 0: doc id i has no ordinal in the
 * index's doc table and its row is empty (a doc removed by an incremental refresh keeps its ordinal and has no
 * posting left: found 1, matches 0 -- the host's doc table tells it from a live doc).  A doc id given twice is answered once and copied.  The impacts of `algo`
 * are materialised on demand, as by a search.  0 / -1.
 *
 * There is no forward index: every term's list is asked for the docs (csrc/nxs_docterms.h, on top of
 * nxs_explain.h's searches).  k_dv_ord finds the ordinals; k_dv_scan -- (part of the term-id range, chunk of
 * at most 64 docs by ascending ordinal) per wavefront, at most NXS_GPU_DOCTERMS_PARTS (default 512) parts --
 * matches each list with the chunk from the shorter side, counts eligible hits and keeps a running top-k per
 * doc in LDS; k_dv_merge selects the k best of a doc's parts and reads w, tf and df at their postings.
 * Device memory is docs x parts x k keys, never a list of hits; a batch whose partial lists would exceed
 * NXS_GPU_DOCTERMS_WS (default 64 MiB) is cut into passes of whole chunks.  The pass has a stream, a grow-only workspace, pinned staging and
 * events of its own: allowed while batches and fuzzy passes are in flight, takes none of their slots;
 * blocking.  An index that is never asked allocates, uploads and launches nothing.  Under
 * NXS_GPU_DOCTERMS=host (the cross-check route) the posting arrays are copied back and the same lookups and a
 * plain sort run on the host.
 *
 * nxsgpu_doc_terms_profile: since the last reset -- out[0] calls that reached the device, out[1] / out[2] /
 * out[3] HIP-event ms of k_dv_ord / k_dv_scan / k_dv_merge (with nxsgpu_set_profiling only), out[4] passes,
 * out[5] distinct live docs answered on the device, out[6] docs answered on the host, out[7] eligible
 * (term, doc) pairs counted on the device.
 */
#define	NXSGPU_DOCTERMS_MAX	32
#define	NXSGPU_DOCTERMS_PROF	8
int		nxsgpu_doc_terms(nxsgpu_index_t *, int algo, const uint64_t *doc_ids, uint32_t n, uint32_t mindf, uint32_t k,
		    uint32_t *term_ids, float *w, uint32_t *tf, uint32_t *df,	/* rows [n][k] */
		    uint32_t *counts, uint32_t *matches, uint8_t *found);	/* [n]; found 0 = not a live doc */
void		nxsgpu_doc_terms_profile(nxsgpu_index_t *, double out[NXSGPU_DOCTERMS_PROF], int reset);

/*
 * ---- related terms of a query's matches -----------------------------------------------
 *
 * nxsgpu_related: for each of n plans the doc set M of the plan's expression -- exactly what nxsgpu_count counts:
 * live docs, empty under a ranking function that scores nothing -- and the ELIGIBLE terms: c = the docs of M that
 * hold the term (membership: a doc counts once whatever its tf) >= mincount, the live df (the length of the
 * term's list, what nxsgpu_index_df reports) >= mindf, and, unless `self`, not one of the plan's own term_id[].
 * order 0 ("count"): c descending, term id ascending; order 1 ("share"): s = (float)((double)c / (double)df)
 * descending as floats, term id ascending (csrc/nxs_related.h).  Rows of k (1..NXSGPU_RELATED_MAX) entries:
 * term_ids / count / df [n][k], counts[i] = min(k, matches[i]), matches[i] the exact number of eligible terms,
 * docs[i] = |M|.  A plan that is empty or matches nothing has docs 0 and an empty row.  Identical plans are
 * answered once and copied.  No impact is read: nothing is materialised.  0 / -1.
 *
 * A pass serves a group of G <= 32 distinct plans: k_rt_mask writes the doc sets as bits (a u32 per doc ordinal;
 * k_count_tile's body with one more ending), k_rt_scan streams the posting array ONCE per group -- a workgroup per
 * run of NXS_GPU_RELATED_RUN (default 4096; a multiple of 64, 64 at least) postings, a lane per posting gathers its
 * doc's word, a wavefront that finds none set moves on, the others add one popcount per (segment of equal terms,
 * plan bit) into c[g][term] --, k_rt_select keeps a top-k per part of a plan's count row (at most
 * NXS_GPU_RELATED_PARTS, default 64, parts), k_rt_merge merges the parts.  The count rows of a group are bounded
 * by NXS_GPU_RELATED_WS (default NXSGPU_RELATED_WS = 256 MiB: 32 rows of up to 2 M terms): G is what fits, one
 * row at least, and a batch is cut into passes of G plans.  The pass has a stream, a grow-only workspace, pinned
 * staging and events of its own: allowed while batches and fuzzy passes are in flight, takes none of their
 * slots; blocking.  An index that is never asked allocates, uploads and launches nothing.  Under
 * NXS_GPU_RELATED=host (the cross-check route) the posting array is copied back, the doc set is evaluated from
 * the plan's postfix program on the host, the counts are taken by a plain loop and ranked by nxs_rt_rank.
 *
 * nxsgpu_related_profile: since the last reset -- out[0] distinct plans answered on the device, out[1] on the
 * host, out[2] passes, out[3] / out[4] / out[5] / out[6] HIP-event ms of k_rt_mask / k_rt_scan / k_rt_select /
 * k_rt_merge (with nxsgpu_set_profiling only), out[7] calls that had a plan to answer.
 */
#define	NXSGPU_RELATED_MAX	32
#define	NXSGPU_RELATED_PROF	8
#define	NXSGPU_RELATED_WS	(256ull << 20)
int		nxsgpu_related(nxsgpu_index_t *, int algo, const nxsgpu_query_t *plans, uint32_t n, int order,
		    uint32_t mindf, uint32_t mincount, int self, uint32_t k,
		    uint32_t *term_ids, uint32_t *count, uint32_t *df,		/* rows [n][k] */
		    uint32_t *counts, uint32_t *matches, uint32_t *docs);	/* [n] */
void		nxsgpu_related_profile(nxsgpu_index_t *, double out[NXSGPU_RELATED_PROF], int reset);

/*
 * ---- search within a doc-id set ---------------------------------------------------------
 *
 * nxsgpu_search_docs: for each of n plans the results of the plan restricted to its set -- sets[set_of[i]], set_len
 * ids, ASCENDING AND DISTINCT (csrc/nxs_docset.h: nxs_ds_sort_unique), at most NXSGPU_DOCSET_MAX; an id that is not
 * in the doc table is ignored, a removed doc keeps its ordinal and matches nothing.  A doc of the set is a result
 * when the plan's expression holds on its presence mask and at least one present token has a non-negative float;
 * its score is the f32 sum of those floats in ascending token order (the REGULAR posting of a TF-IDF dense term,
 * as nxsgpu_explain reads it).  The results are fed in descending doc id into the reference's capped heap of
 * `limit` (>= 1, any value) entries and sorted by its heap_sort (k_replay): res as nxsgpu_search fills it;
 * totals[n] (may be NULL) = the results before the cap.  The impacts of `algo` are materialised on demand.  0 / -1.
 *
 * A plan of more than 8 tokens is evaluated from its postfix program on a 64-bit stack: a program that names a token
 * >= n_tokens, underflows, leaves nothing or is deeper than 64 fails the call (nxs_ds_prog_ok; what the host's
 * compiler emits never is).
 *
 * The scoring is driven from the docs (|set| x tokens lookups; no list is streamed).  k_ds_ord resolves the ids of
 * the call's distinct sets to ordinals ONCE, before the passes: the ids go up in slices, the ordinals stay on the host
 * (4 B an id).  k_ds_score -- a wavefront per (query, chunk of NXS_GPU_DOCSET_CHUNK, default 1024, a multiple of 64,
 * entries), a lane per doc, the token loop wave-uniform -- compacts the matches of a chunk into its candidate segment in
 * descending doc order, and the replay takes the segments from the last to the first: the heap across the lanes up to
 * limit 64, in LDS up to 8000, in global memory with capacity min(limit, |set|) beyond.  A pass serves whole queries,
 * one at least, within NXS_GPU_DOCSET_WS (default NXSGPU_DOCSET_WS) bytes of workspace, and uploads the ordinals of
 * the sets its queries use.  The call has a stream, a grow-only workspace, pinned staging and events of its own:
 * allowed while batches and fuzzy passes are in flight, takes none of their slots; blocking.  An index that is never
 * asked allocates, uploads and launches nothing.  Under NXS_GPU_DOCSET=host (the cross-check route) the index arrays
 * are copied back, the ordinals and every (query, doc) are evaluated on the host by the same nxs_ds_lane, and the
 * candidates go through the same device replay.
 *
 * nxsgpu_search_docs_profile: since the last reset -- out[0] calls that reached the device, out[1] passes, out[2]
 * distinct sets resolved, out[3] ids resolved, out[4] / out[5] (query, doc) cells scored on the device / on the
 * host, out[6] candidates, out[7] / out[8] / out[9] HIP-event ms of k_ds_ord / k_ds_score / k_replay (with
 * nxsgpu_set_profiling only).
 */
#define	NXSGPU_DOCSET_MAX	(1u << 22)
#define	NXSGPU_DOCSET_PROF	12
#define	NXSGPU_DOCSET_WS	(256ull << 20)
int		nxsgpu_search_docs(nxsgpu_index_t *, int algo, uint64_t limit, const nxsgpu_query_t *plans, uint32_t n,
		    const uint64_t *const *sets, const uint32_t *set_len, uint32_t n_sets, const uint32_t *set_of,
		    nxsgpu_results_t *res, uint32_t *totals);
void		nxsgpu_search_docs_profile(nxsgpu_index_t *, double out[NXSGPU_DOCSET_PROF], int reset);

/*
 * ---- a query's matches listed by doc id ---------------------------------------------------
 *
 * nxsgpu_match_docs: for each of n plans the doc set M of the plan's expression -- exactly what nxsgpu_count counts
 * and what nxsgpu_related calls M: live docs, empty under a ranking function that scores nothing -- as a PAGE: the
 * docs of M whose id is >= from[i], in ascending doc id, the first `limit` (1..NXSGPU_MATCH_MAX) of them.  ids is
 * [n][cap] with cap = min(limit, nxsgpu_index_docs()); row i holds counts[i] ids, more[i] = a doc of M lies beyond
 * the page, totals[i] = |M| whatever the cursor.  A plan that is empty or matches nothing has counts 0 and totals
 * 0.  (plan, from) pairs that are identical are answered once and copied.  No impact is read: nothing is
 * materialised.  A plan of more than 8 tokens is evaluated from its postfix program: a program that nxs_ds_prog_ok
 * (csrc/nxs_docset.h) refuses fails the call.  0 / -1.
 *
 * Doc ordinals ascend with doc ids, so a page is a stream compaction of M's bits.  A pass serves a group of G <= 32
 * distinct pairs: k_md_mask writes the doc sets as bits (a u32 per doc ordinal; k_count_tile's body, as k_rt_mask),
 * k_md_from turns the cursors into ordinals (a lower bound over the doc ids, csrc/nxs_matchdocs.h), k_md_count --
 * a wavefront per run of NXS_GPU_MATCHDOCS_RUN (default 256; a multiple of 64, 64..65536) ordinals -- counts every
 * pair's docs at or beyond its cursor per run by ballot, one plain store per (pair, run), k_md_scan turns a pair's
 * row into ranks (one workgroup per pair), k_md_emit walks the runs again and stores the doc id of every match
 * whose rank is below the limit at ids[g][rank]: ascending and deterministic by construction.  Per pass: 4 B a doc
 * for the masks, 4 B per (pair, run), 8 B x cap per pair, within NXS_GPU_MATCHDOCS_WS (default
 * NXSGPU_MATCHDOCS_WS) bytes: G is what fits, one pair at least, and a batch is cut into passes of G pairs.  The
 * pass has a stream, a grow-only workspace, pinned staging and events of its own: allowed while batches and fuzzy
 * passes are in flight, takes none of their slots; blocking.  An index that is never asked allocates, uploads and
 * launches nothing.  Under NXS_GPU_MATCHDOCS=host (the cross-check route) the posting array and the doc ids are
 * copied back, the doc set is evaluated from the plan's postfix program on the host and the page is nxs_md_page's.
 *
 * nxsgpu_match_docs_profile: since the last reset -- out[0] distinct pairs answered on the device, out[1] on the
 * host, out[2] passes, out[3] ids emitted, out[4] .. out[8] HIP-event ms of k_md_mask / k_md_from / k_md_count /
 * k_md_scan / k_md_emit (with nxsgpu_set_profiling only), out[9] calls that had a pair to answer.
 */
#define	NXSGPU_MATCH_MAX	(1u << 22)
#define	NXSGPU_MATCHDOCS_PROF	10
#define	NXSGPU_MATCHDOCS_WS	(256ull << 20)
int		nxsgpu_match_docs(nxsgpu_index_t *, int algo, const nxsgpu_query_t *plans, uint32_t n,
		    const uint64_t *from /* [n] */, uint32_t limit, uint64_t *ids /* [n][cap] */,
		    uint32_t *counts, uint8_t *more, uint32_t *totals);		/* [n] */
void		nxsgpu_match_docs_profile(nxsgpu_index_t *, double out[NXSGPU_MATCHDOCS_PROF], int reset);

/*
 * ---- host batches as fixed-size records; query sharding over several GPUs ----
 *
 * The reference scales out by running independent worker processes
 * (compose/nginx.conf:2); here a batch shards BY QUERY over the GPUs of a node
 * (SURVEY.md 8e): every rank holds a replica of the device index, takes a
 * contiguous slice of the batch, and ONE RCCL all-gather of fixed-size
 * per-query records reassembles the batch on every rank.
 *
 * Record of one query (limit k <= NXSGPU_BIG_K), NXSGPU_REC_BYTES(k) bytes:
 *	u32 count | u32 flags | u64 doc_id[k] | f32 score[k] | pad to 8
 * A rank's BLOCK = n_slots records followed by n_slots + 1 u32 status words:
 * one per slot (the nxs_err_t of a query that never reached the device) and a
 * last word of per-rank flags every rank reads after the all-gather
 * (NXSGPU_BLOCK_CHANGED), padded to 8 bytes.
 * With one rank there is no collective and the block is simply the batch's
 * host copy.
 */
#define	NXSGPU_REC_BYTES(k)	((8 + 12 * (size_t)(k) + 7) & ~(size_t)7)
#define	NXSGPU_STATUS_WORDS(n_slots)	((size_t)(n_slots) + 1)
#define	NXSGPU_BLOCK_BYTES(n_slots, k) \
	((size_t)(n_slots) * NXSGPU_REC_BYTES(k) + ((NXSGPU_STATUS_WORDS(n_slots) * 4 + 7) & ~(size_t)7))
/* block flags word: this rank saw the index files move when it planned the batch --
 * all ranks then re-sync at the same later _begin (nxs.h, "sharded mode") */
#define	NXSGPU_BLOCK_CHANGED	1u
#define	NXSGPU_REC_INEXACT	1u	/* flags: the query needs the exact two-pass path (nxsgpu_search) */
#define	NXSGPU_UID_BYTES	128	/* = NCCL_UNIQUE_ID_BYTES */

typedef struct nxsgpu_comm nxsgpu_comm_t;

/* contiguous slice [lo, hi) of an n-query batch owned by `rank`, and the
 * largest slice (= n_slots of every rank's block) */
void		nxsgpu_shard_slice(uint64_t n, int rank, int world, uint64_t *lo, uint64_t *hi);
uint64_t	nxsgpu_shard_capacity(uint64_t n, int world);

/*
 * One RCCL communicator over the ranks' GPUs.  Rank 0 obtains the unique id,
 * the application hands its bytes to the other ranks (MPI, a file, a socket,
 * torch.distributed ...), then EVERY rank calls nxsgpu_comm_create (collective).
 * librccl is loaded on first use; single-GPU users never touch it.
 */
int		nxsgpu_comm_unique_id(uint8_t uid[NXSGPU_UID_BYTES]);
nxsgpu_comm_t *	nxsgpu_comm_create(int device, int rank, int world,
		    const uint8_t uid[NXSGPU_UID_BYTES]);
void		nxsgpu_comm_destroy(nxsgpu_comm_t *);
int		nxsgpu_comm_rank(const nxsgpu_comm_t *);
int		nxsgpu_comm_world(const nxsgpu_comm_t *);
/* what RCCL itself reports for the communicator (ncclCommCount; -1: unknown), and how much has gone through
 * it: out[0] all-gathers queued, out[1] bytes this rank contributed -- evidence for scaling records */
int		nxsgpu_comm_rccl_count(const nxsgpu_comm_t *);
void		nxsgpu_comm_stats(const nxsgpu_comm_t *, uint64_t out[2]);
/* blocking all-gather of host buffers (staged through the device): the rare
 * fix-up round of a sharded batch, barriers */
int		nxsgpu_comm_allgather(nxsgpu_comm_t *, const void *send, void *recv,
		    size_t bytes_per_rank);
/* batches of this index all-gather their record blocks over `comm` (NULL: detach) */
int		nxsgpu_index_set_comm(nxsgpu_index_t *, nxsgpu_comm_t *);

typedef struct {
	uint32_t	n_slots;	/* records per block */
	uint32_t	k;
	uint32_t	world;		/* blocks */
	size_t		rec_bytes, block_bytes;
	const uint8_t *	blocks;		/* host memory, valid until NXSGPU_INFLIGHT more batches have begun */
} nxsgpu_batch_view_t;

/*
 * Pipelined host batches (up to NXSGPU_INFLIGHT in flight, shared with
 * nxsgpu_search_dev_begin): the result of plans[i] goes to record
 * slot_of_plan[i] of this rank's block; status[NXSGPU_STATUS_WORDS(n_slots)]
 * (NULL: zeros) travels with it.
 * _begin() queues upload, cursors, scans, heap replays, the all-gather (if
 * `gather` is set and a communicator is attached: every rank must then call
 * with the same n_slots and limit) and the copy to pinned host memory, then
 * returns; _end() waits for
 * the OLDEST batch in flight and hands out the blocks.  0 / -1.
 */
int		nxsgpu_batch_begin(nxsgpu_index_t *, int algo, uint32_t limit,
		    const nxsgpu_query_t *plans, uint32_t n_plans,
		    const uint32_t *slot_of_plan, const uint32_t *status,
		    uint32_t n_slots, int gather);
int		nxsgpu_batch_end(nxsgpu_index_t *, nxsgpu_batch_view_t *);

/*
 * ---- total match counts ----------------------------------------------------------
 *
 * total of a query = the cardinality of the reference's expression bitmap
 * (get_expr_bitmap, src/query/search.c:118-174): how many docs the query would
 * return with an unbounded limit.  It does not depend on the limit or -- apart from
 * a ranking function that scores nothing (BM25 on an index whose header says
 * adl < 1: total 0) -- on the ranking function.  The top-k paths skip most matching
 * docs on purpose, so the count is a pass of its own over the doc ordinals of the
 * primary CSR (nxs_gpu_count.hip: k_count_tile, k_count_req): no impacts, no heap.
 *
 * nxsgpu_count       blocking, totals[n] on the host, fixed-size plans
 * nxsgpu_count_wide  the same for plans beyond nxsgpu_query_t (k_scanw's count pass)
 * nxsgpu_search_totals  nxsgpu_search() that also delivers totals[n]: queries that
 *                    take the exact two-pass path report what its count pass
 *                    matched, the others are counted by the count kernels
 * nxsgpu_search_wide_totals  nxsgpu_search_wide() likewise (always the exact path)
 * nxsgpu_batch_begin_opts  nxsgpu_batch_begin() with options: `totals` queues the
 *                    count kernels on a stream of the batch, beside its scans;
 *                    nxsgpu_batch_end_totals() then also hands out totals[n_plans]
 *                    (plan order; host memory, valid as long as the view's blocks).
 *                    Not with `gather`: a sharded batch's totals would have to
 *                    travel in the record blocks every rank agrees on (-1).
 * NXS_GPU_COUNT=auto|tile|req|scan picks the route: by the query's shape (auto: the
 * driver kernel where a token is required, else the exact path's count pass),
 * the tile kernel for everything, the driver kernel wherever a token is required
 * and the tile kernel for the rest, or the exact path's own count pass (MODE_COUNT)
 * for everything: the cross-check and baseline.
 */
typedef struct {
	int		totals;		/* count every plan's matches */
} nxsgpu_batch_opts_t;

int		nxsgpu_count(nxsgpu_index_t *, int algo, const nxsgpu_query_t *queries,
		    uint32_t n_queries, uint32_t *totals);
int		nxsgpu_count_wide(nxsgpu_index_t *, int algo, const nxsgpu_wide_query_t *queries,
		    uint32_t n_queries, uint32_t *totals);
int		nxsgpu_search_totals(nxsgpu_index_t *, int algo, uint64_t limit,
		    const nxsgpu_query_t *queries, uint32_t n_queries,
		    nxsgpu_results_t *res, uint32_t *totals);
int		nxsgpu_search_wide_totals(nxsgpu_index_t *, int algo, uint64_t limit,
		    const nxsgpu_wide_query_t *queries, uint32_t n_queries,
		    nxsgpu_results_t *res, uint32_t *totals);
int		nxsgpu_batch_begin_opts(nxsgpu_index_t *, int algo, uint32_t limit,
		    const nxsgpu_query_t *plans, uint32_t n_plans,
		    const uint32_t *slot_of_plan, const uint32_t *status,
		    uint32_t n_slots, int gather, const nxsgpu_batch_opts_t *opts);
int		nxsgpu_batch_end_totals(nxsgpu_index_t *, nxsgpu_batch_view_t *, const uint32_t **totals);
/* docs per LDS tile of k_count_tile: out[0] with byte masks (<= 8 tokens), out[1] with word masks */
void		nxsgpu_count_tile_widths(uint32_t out[2]);
/* profiling (nxsgpu_set_profiling): HIP-event time of the count kernels alone since the last reset --
 * out[0] / out[1] launches and ms of k_count_tile, out[2] / out[3] of k_count_req, out[4] / out[5] the
 * queries routed to each */
void		nxsgpu_count_profile(nxsgpu_index_t *, double out[6], int reset);
/* number of batches in flight (either API) */
int		nxsgpu_batches_in_flight(const nxsgpu_index_t *);

/*
 * The caller's worker threads for the host side of a batch (per-query plan -> device form:
 * embarrassingly parallel, 0.15 ms on one thread for 1024 five-term queries): `run` executes
 * body(arg, lo, hi) over [0, n) in chunks on whatever threads it has and returns when all of it
 * is done.  NULL: one thread.  nxs_pool.c hands over the nxs_t's pool (the one that parses).
 */
typedef void (*nxsgpu_body_t)(void *arg, size_t lo, size_t hi);
typedef void (*nxsgpu_parallel_t)(void *ctx, nxsgpu_body_t body, void *arg, size_t n, size_t chunk);
void		nxsgpu_index_set_parallel(nxsgpu_index_t *, nxsgpu_parallel_t run, void *ctx);

/* re-read the NXS_GPU_* switches (they are parsed once at index create);
 * tests and A/B tools only */
void		nxsgpu_index_reconfigure(nxsgpu_index_t *);

/*
 * Measured HBM roofline on THIS device: streams the index's own posting array
 * (16 B per lane, every CU busy) `reps` times and reports the best read rate in
 * GB/s, the denominator bench.py prints beside the nominal 8 TB/s.  0 on error.
 */
double		nxsgpu_hbm_read_gbs(nxsgpu_index_t *, int reps);
/* one launch of k_hbm_read (16 B/lane) and of k_hbm_read_x2 (8 B/lane, the scan
 * kernels' width) over *bytes bytes each: known byte counts to calibrate the
 * FETCH_SIZE counter against (tools/pmc_calib.py) */
int		nxsgpu_hbm_calibrate(nxsgpu_index_t *, uint64_t *bytes);

void		nxsgpu_set_profiling(nxsgpu_index_t *, int on);
void		nxsgpu_get_profile(nxsgpu_index_t *, nxsgpu_profile_t *, int reset);
void		nxsgpu_synchronize(nxsgpu_index_t *);

#ifdef __cplusplus
}
#endif
#endif
