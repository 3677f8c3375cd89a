/*
 * nxs_hooks.h -- NOT part of the library's ABI: test hooks (nxs_test_*) and the bench's
 * accessors.  They exist only in builds with -DNXS_TEST_HOOKS (the Makefile's default,
 * which is what tests/ and bench.py load; `make HOOKS=` builds the library without them:
 * the drop-in a consumer of include/nxs.h links).  Python reaches them through ctypes
 * (nxsearch_amd/__init__.py, nxsearch_amd/multi.py).  A hook that reaches a static function is defined in
 * that function's unit, beside what it tests; the ones that reach none are in nxs_hooks.c.
 */
#ifndef NXS_HOOKS_H
#define NXS_HOOKS_H
#ifdef NXS_TEST_HOOKS

#include "nxs_impl.h"

/*
 * Host-side phase times of the batches since the last call, in seconds:
 * out[0] parse/resolve/compile, out[1] queueing on the device, out[2] waiting
 * for the device, out[3] building responses, out[4] number of batches, out[5]
 * queries that had to be re-run on the exact two-pass path, out[6] / out[7] the
 * whole _begin() / _end() calls.
 */
void		nxs_index_host_profile(nxs_index_t *, double out[12]);
/* out[0] ncclCommCount of the attached communicator (-1: none / unknown), out[1] world, out[2] all-gathers queued,
 * out[3] bytes this rank contributed to them */
void		nxs_index_shard_info(nxs_index_t *, uint64_t out[4]);
/* the device-side handle behind an index (nxs_gpu.h): pre-resolved plans, results left in HBM */
struct nxsgpu_index;
struct nxsgpu_index *nxs_index_device(nxs_index_t *);
/*
 * One part of the device index image, read back: scalars, doc tables and CSR, the impacts and per-term maxima of
 * a ranking function, the dense terms' columns (f32 and byte form) with the TF-IDF caps and outlier lists, the
 * block-presence bitmaps and rank directories, a doc shard's collection-wide df (the parts and the scalars' order:
 * nxsgpu_test_index_image in nxs_gpu_index.hip, IMG_* in nxsearch_amd/__init__.py).  *need = the part's bytes, copied to `out` if cap
 * holds them; a part that is not materialised has 0 bytes.  Refused while batches are in flight; waits for the
 * index's streams, copies with hipMemcpy and changes nothing on the device.  0, or -1 with the error declared.
 */
int		nxs_test_index_image(nxs_index_t *, int part, int algo, void *out, size_t cap, size_t *need);
/* ... its device half (nxs_gpu_index.hip); the error is nxsgpu_last_error() */
int		nxsgpu_test_index_image(struct nxsgpu_index *, int part, int algo, void *out, size_t cap, size_t *need);
/*
 * One part of the term-side device state, read back under the same rules: the BK image (nodes, byte pool), the
 * side arrays of the match-first fuzzy search (parent, slot) and its candidates (node, signature, length, the first
 * candidate of every length), suggest's candidates, and the byte order of the live terms with its selection keys
 * that completion and wildcard matching read (the parts and the scalars' order: nxsgpu_test_term_image in
 * nxs_gpu_fuzzy.hip, which reaches the order through nxs_gpu_prefix.hip; TIMG_* in nxsearch_amd/__init__.py).
 * Builds nothing: a lazily built state that is behind its generation comes back as it is, and says so in the scalars.
 */
int		nxs_test_term_image(nxs_index_t *, int part, void *out, size_t cap, size_t *need);
int		nxsgpu_test_term_image(struct nxsgpu_index *, int part, void *out, size_t cap, size_t *need);
/* the plan cache (query string -> compiled plan) on / off at run time */
void		nxs_index_set_plan_cache(nxs_index_t *, int on);

/* worker pool: every item of every run worked on exactly once */
size_t		nxs_test_pool(unsigned n_thr, size_t n, unsigned rounds, size_t chunk);
/* parser / plan compiler without an index */
char *		nxs_test_query_repr(const char *query, char **errmsg);
int		nxs_test_compile(const char *query, const char *const *words, uint32_t n_words,
		    bool lowercase, nxsgpu_query_t *plan, int *empty, char *err, size_t errlen);
int		nxs_test_compile_wide(const char *query, const char *const *words, uint32_t n_words,
		    int *wide, uint32_t *n_tokens, uint32_t *term_ids, uint32_t cap_t,
		    uint32_t *prog_len, uint16_t *prog, uint32_t cap_p);
char *		nxs_test_filter(const char *basedir, int stages, const char *s, int *act);
int		nxs_test_bk_image(const char *const *words, uint32_t n_words, nxs_bkimage_t *out);
int		nxs_test_levdist(const uint8_t *a, size_t n, const uint8_t *b, size_t m);
/* query sharding without a second GPU: one emulated rank, record blocks, the fix-up protocol */
void		nxs_test_shard_emulate(nxs_index_t *, int rank, int world);
size_t		nxs_test_shard_block(nxs_index_t *, uint8_t *out, size_t cap);
void		nxs_test_pack_record(uint8_t *block, uint32_t n_slots, uint32_t k, uint32_t slot,
		    uint32_t count, const uint64_t *ids, const float *scores, uint32_t status);
void		nxs_test_mark_inexact(uint8_t *block, uint32_t n_slots, uint32_t k, uint32_t slot);
void		nxs_test_mark_changed(uint8_t *block, uint32_t n_slots, uint32_t k);
int		nxs_test_blocks_changed(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k);
void		nxs_test_pack_abort(uint8_t *block, uint32_t n_slots, uint32_t k, uint32_t code);
int		nxs_test_fixup_scan(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k,
		    size_t n, int rank, uint32_t *which, size_t *nw);
int		nxs_test_fixup_verify(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k, size_t n);
int		nxs_test_assemble(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k,
		    size_t n, nxs_resp_t **resps, nxs_err_t *errs, int only_rank);
void		nxs_test_inject_failure(nxs_index_t *, int which, unsigned nth);
/* doc shards: the two halves of the rank form */
int		nxs_test_docshard_block(nxs_index_t *shard, nxs_params_t *, const char *const *queries, size_t n,
		    uint32_t cap, uint8_t **block, size_t *len);
int		nxs_test_docshard_finish(nxs_index_t *shard, nxs_params_t *, const char *const *queries, size_t n,
		    uint32_t cap, const uint8_t *gathered, nxs_resp_t **resps, nxs_err_t *errs);
int		nxs_test_docshard_set_df(nxs_index_t *const *shards, unsigned n_shards);
/* doc shards: the phases of nxs_docshard_refresh_rank() between its collectives, the agreement rule */
void		nxs_test_docshard_refresh_record(nxs_index_t *shard, uint64_t rec[8]);
int		nxs_test_docshard_refresh_merge(nxs_index_t *shard, const uint64_t *recs, unsigned W,
		    uint8_t **block, size_t *len);
uint32_t	nxs_test_docshard_refresh_finish(nxs_index_t *shard, const uint8_t *gathered, unsigned W, size_t len);
int		nxs_test_docshard_refresh_settle(nxs_index_t *shard, const uint32_t *fin, unsigned W);
int		nxs_test_docshard_agree(const uint64_t *recs, unsigned W, const uint64_t consumed[4], uint64_t out[8]);
uint64_t	nxs_test_impact_passes(nxs_index_t *);
/* total match counts: docs per LDS tile of k_count_tile -- out[0] byte masks (<= 8 tokens), out[1] word masks
 * (tests straddle them) */
void		nxs_test_count_tile_widths(uint32_t out[2]);
/* spelling suggestions: the host ranker (nxs_suggest.h) over a dictionary handed in (term i has id i + 1;
 * out_*: room for k), the parameters as nxs_index_suggest reads them (0, or -1 with the error declared), and
 * an nxs_sugg_t built by hand (accessors and JSON without an index) */
void		nxs_test_suggest_host(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs,
		    uint32_t n_terms, const uint8_t *token, size_t len, uint32_t maxdist, uint32_t k,
		    uint32_t *out_ids, uint8_t *out_dist, uint32_t *out_df, uint32_t *count, uint32_t *matches);
int		nxs_test_suggest_params(nxs_t *, nxs_params_t *, unsigned *k, unsigned *maxdist);
nxs_sugg_t *	nxs_test_sugg_build(const char *token, size_t token_len, bool dropped, uint64_t matches,
		    unsigned count, const uint8_t *const *terms, const size_t *lens, const unsigned *dists,
		    const uint64_t *dfs);

/* prefix completion: the host ranker (nxs_complete.h) over a dictionary handed in (term i has id i + 1), the
 * parameters as nxs_index_complete and a search read them, a completion object built by hand, a query's
 * prefix leaves marked, resolved with the host ranker and spliced (-> nxs_query_repr of the result), and the
 * filter stages a prefix takes */
void		nxs_test_complete_host(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs,
		    uint32_t n_terms, const uint8_t *prefix, size_t len, uint32_t k,
		    uint32_t *out_ids, uint32_t *out_df, uint32_t *count, uint32_t *matches);
int		nxs_test_complete_params(nxs_t *, nxs_params_t *, unsigned *k, int *prefixmatch, unsigned *prefix_limit);
nxs_sugg_t *	nxs_test_compl_build(const char *prefix, size_t prefix_len, uint64_t matches, unsigned count,
		    const uint8_t *const *terms, const size_t *lens, const uint64_t *dfs);
char *		nxs_test_prefix_query(const char *query, const char *const *words, const uint32_t *dfs,
		    uint32_t n_words, bool lowercase, bool prefixmatch, uint32_t prefix_limit, uint32_t *n_prefix,
		    char *prefixes, size_t cap);
char *		nxs_test_filter_prefix(const char *basedir, int stages, const char *s, int *act);

/* wildcard matching: the matcher alone (nxs_wild.h; _inl: as the device runs it, the first 8 bytes from an inline
 * copy), the host ranker over a dictionary handed in (term i has id i + 1), the parameters as
 * nxs_index_wildcard and a search read them, a wildcard object built by hand, and a query's prefix and
 * wildcard leaves marked, resolved with the host rankers and spliced (-> nxs_query_repr of the result;
 * `leaves`: a line `p <prefix>` or `w <pattern>` per leaf, source order) */
int		nxs_test_wild_match(const uint8_t *term, size_t tlen, const uint8_t *pat, size_t plen);
int		nxs_test_wild_match_inl(const uint8_t *term, size_t tlen, const uint8_t *pat, size_t plen);
void		nxs_test_wild_host(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs,
		    uint32_t n_terms, const uint8_t *pat, size_t len, uint32_t k,
		    uint32_t *out_ids, uint32_t *out_df, uint32_t *count, uint32_t *matches);
int		nxs_test_wild_params(nxs_t *, nxs_params_t *, unsigned *k, int *wildcardmatch, unsigned *wildcard_terms);
/* ... a pattern of `len` bytes as the call normalises it (nxs_wild_normalize's result; out: at most cap bytes) */
int		nxs_test_wild_normalize(bool lowercase, const char *pat, size_t len, char *out, size_t cap,
		    size_t *out_len, size_t *literals);
nxs_sugg_t *	nxs_test_wild_build(const char *pattern, size_t pattern_len, uint64_t matches, unsigned count,
		    const uint8_t *const *terms, const size_t *lens, const uint64_t *dfs);
char *		nxs_test_wild_query(const char *query, const char *const *words, const uint32_t *dfs,
		    uint32_t n_words, bool lowercase, bool prefixmatch, bool wildcardmatch, uint32_t prefix_limit,
		    uint32_t wildcard_terms, uint32_t *n_leaves, char *leaves, size_t cap, int *errcode);

/* explanations: the "explain" key as a search reads it, a response built by hand from given arrays (accessors
 * and the JSON writer without an index; cells [count][n_tok], tf == 0 = absent), and the searches of the shared
 * header nxs_explain.h over a list handed in (pos: nxs_ex_find, UINT64_MAX = absent; lower: nxs_ex_lower;
 * bitmap: through a block bitmap + rank directory built from the list) */
int		nxs_test_explain_params(nxs_t *, nxs_params_t *, int *explain);
nxs_resp_t *	nxs_test_resp_build(unsigned count, const uint64_t *ids, const float *scores, bool has_total,
		    uint64_t total, bool explained, unsigned n_tok, const uint8_t *const *terms, const size_t *lens,
		    const uint32_t *tf, const float *imp);
int		nxs_test_explain_search(const uint64_t *dt, uint64_t n, bool bitmap, uint32_t n_docs,
		    const uint32_t *docs, size_t nd, uint64_t *pos, uint64_t *lower);
void		nxs_test_explain_ordinal(const uint64_t *ids, uint64_t n, const uint64_t *q, size_t nq, uint64_t *out);


/* similar documents: the parameters as nxs_index_doc_terms / nxs_index_similar read them (0, or -1 with the error
 * declared), an nxs_sugg_t of the term-vector kind built by hand, the lookups of the shared header
 * nxs_docterms.h over a list handed in (one list against one chunk of ascending ordinals: pos[j] = the position
 * of ordinal j's posting, UINT64_MAX = absent; by_posting: 1 / 0 force the side the searches start from, -1 the
 * rule of the kernel; bitmap: through a block bitmap + rank directory built from the list; -> the side taken),
 * nxs_dv_key, and nxs_index_similar's self-removal on a response built by nxs_test_resp_build */
int		nxs_test_docterms_params(nxs_t *, nxs_params_t *, unsigned *k, unsigned *mindf, unsigned *similar_terms,
		    unsigned *similar_mindf, int *similar_self);
nxs_sugg_t *	nxs_test_docterms_build(uint64_t doc, uint64_t matches, unsigned count, const uint8_t *const *terms,
		    const size_t *lens, const unsigned *tfs, const uint64_t *dfs, const float *scores);
int		nxs_test_docterms_lane(const uint64_t *dt, uint64_t n, bool bitmap, uint32_t n_docs, const uint32_t *ords,
		    uint32_t nd, int by_posting, uint64_t *pos);
uint64_t	nxs_test_docterms_key(float w, uint32_t term);
void		nxs_test_similar_drop(nxs_resp_t *, uint64_t doc, uint64_t limit);


/* related terms: nxs_index_related's own parameters as it reads them (0, or -1 with the error declared), an
 * nxs_sugg_t of the related kind built by hand (distance = c, the score is the share), and nxs_related.h: the key
 * of (c, df, term) under order 0 ("count") / 1 ("share"), the share, the eligibility predicate and the host
 * ranker over c[t], df[t], t = 1 .. n_terms (-> rows written, *matches exact; -1: out of memory) */
int		nxs_test_related_params(nxs_t *, nxs_params_t *, unsigned *k, int *order, unsigned *mindf,
		    unsigned *mincount, int *self);
nxs_sugg_t *	nxs_test_related_build(const char *query, size_t query_len, uint64_t docs, uint64_t matches,
		    unsigned count, const uint8_t *const *terms, const size_t *lens, const unsigned *cs,
		    const uint64_t *dfs);
uint64_t	nxs_test_related_key(int order, uint32_t c, uint32_t df, uint32_t term);
float		nxs_test_related_share(uint32_t c, uint32_t df);
bool		nxs_test_related_eligible(uint32_t c, uint32_t df, uint32_t mincount, uint32_t mindf, uint32_t term,
		    const uint32_t *excl, uint32_t n_excl);
int		nxs_test_related_rank(int order, const uint32_t *c, const uint32_t *df, uint32_t n_terms, uint32_t mincount,
		    uint32_t mindf, const uint32_t *excl, uint32_t n_excl, uint32_t k, uint32_t *out_ids,
		    uint64_t *matches);

/* search within a doc-id set: nxs_ds_sort_unique on ids[0 .. n) in place (-> how many are left), and nxs_ds_lane
 * (nxs_docset.h) over arrays handed in, in the style of nxs_test_docterms_lane: nt lists back to back in dt / imp
 * (list j = positions off[j] .. off[j + 1]; dt entries doc << 32 | tf, ascending by doc, docs below n_docs; imp
 * the float of the same position), the plan's truth table and postfix program, nd doc ordinals; bitmap: every list
 * through a block bitmap + rank directory built from it.  hit[i] / score[i]: the lane's answer for ords[i].  0 / -1 */
size_t		nxs_test_docset_sort(uint64_t *ids, size_t n);
int		nxs_test_docset_lane(const uint64_t *dt, const float *imp, const uint64_t *off, uint32_t nt, bool bitmap,
		    uint32_t n_docs, const uint32_t *truth, const uint8_t *prog, uint32_t prog_len, const uint32_t *ords,
		    size_t nd, uint8_t *hit, float *score);

/* a query's matches by doc id: nxs_index_match_docs' own parameters as it reads them (0, or -1 with the error
 * declared), an nxs_docs_t built by hand, and nxs_matchdocs.h over caller arrays: the lower bound of `from` in
 * ids[0 .. n), and a page of the set in_bits ((D + 31) / 32 words, a bit per doc ordinal) -> ids written to out
 * (room for min(limit, D)), *more = a doc of the set lies beyond them */
int		nxs_test_match_params(nxs_t *, nxs_params_t *, unsigned *limit, uint64_t *from);
nxs_docs_t *	nxs_test_docs_build(const char *query, const uint64_t *ids, size_t count, uint64_t total, bool more);
uint64_t	nxs_test_md_lower_bound(const uint64_t *ids, uint64_t n, uint64_t from);
uint64_t	nxs_test_md_page(const uint32_t *in_bits, const uint64_t *doc_ids, uint64_t D, uint64_t from,
		    uint64_t limit, uint64_t *out, bool *more);

#endif /* NXS_TEST_HOOKS */
#endif /* NXS_HOOKS_H */
