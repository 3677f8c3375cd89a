/*
 * nxs.h -- query-side C API of the MI355X-native nxsearch ranking engine.
 *
 * Drop-in for the query path of the reference's public header
 * (reference src/core/nxs.h:21-101, docs/c-api.md:113-148): same names,
 * signatures, ownership and error conventions, so that a program linked
 * against libnxsearch can be relinked against libnxsearch_gpu.so for
 * searching an index that the reference (or anything writing the same
 * on-disk format, src/index/storage.h:13-134) has produced.
 *
 * Not provided (out of scope): index creation and
 * mutation (nxs_index_create/add/remove/destroy), Lua filters.
 *
 * Added: nxs_index_search_batch() -- the reference API is one query per call;
 * a GPU wants many (SURVEY.md 8b last row).
 */
#ifndef NXS_GPU_PUBLIC_H
#define NXS_GPU_PUBLIC_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint64_t nxs_doc_id_t;			/* nxs.h:21 */

struct nxs;
typedef struct nxs nxs_t;

nxs_t *		nxs_open(const char *basedir);	/* nxs.h:26, nxs.c:91-133 */
void		nxs_close(nxs_t *);		/* nxs.h:27 */

/* nxs.h:33-46 -- ABI-frozen codes */
typedef enum {
	NXS_ERR_SUCCESS		= 0,
	NXS_ERR_FATAL,
	NXS_ERR_SYSTEM,
	NXS_ERR_INVALID,
	NXS_ERR_EXISTS,
	NXS_ERR_MISSING,
	NXS_ERR_LIMIT,
} nxs_err_t;

nxs_err_t	nxs_get_error(const nxs_t *, const char **);	/* nxs.h:48 */

/* Parameters (nxs.h:54-67); the query path reads limit / algo / fuzzymatch / total / prefixmatch /
 * prefix_limit / explain / wildcardmatch / wildcard_terms, nxs_index_suggest reads suggest_limit /
 * suggest_maxdist, nxs_index_complete complete_limit, nxs_index_wildcard wildcard_limit, nxs_index_doc_terms
 * docterms_limit / docterms_mindf, nxs_index_similar similar_terms / similar_mindf / similar_self,
 * nxs_index_related related_limit / related_order / related_mindf / related_mincount / related_self,
 * nxs_index_match_docs match_limit / match_from */
struct nxs_params;
typedef struct nxs_params nxs_params_t;

nxs_params_t *	nxs_params_create(void);
/* params.c:201-208: a JSON object of string / unsigned / bool members (how the
 * Lua binding passes limit, algo, fuzzymatch: lua.c:99-110); NULL + NXS_ERR_SYSTEM
 * "params parsing failed: ..." on a syntax error */
nxs_params_t *	nxs_params_fromjson(nxs_t *, const char *, size_t);
int		nxs_params_set_str(nxs_params_t *, const char *, const char *);
int		nxs_params_set_uint(nxs_params_t *, const char *, uint64_t);
int		nxs_params_set_bool(nxs_params_t *, const char *, bool);
void		nxs_params_release(nxs_params_t *);

/* Index handles (nxs.h:73-85): open/close only */
struct nxs_index;
typedef struct nxs_index nxs_index_t;

nxs_index_t *	nxs_index_open(nxs_t *, const char *name);
void		nxs_index_close(nxs_index_t *);

/* Query and response API (nxs.h:87-101) */
struct nxs_resp;
typedef struct nxs_resp nxs_resp_t;

nxs_resp_t *	nxs_index_search(nxs_index_t *, nxs_params_t *,
		    const char *query, size_t len);

void		nxs_resp_iter_reset(nxs_resp_t *);
bool		nxs_resp_iter_result(nxs_resp_t *, nxs_doc_id_t *, float *);
unsigned	nxs_resp_resultcount(const nxs_resp_t *);
char *		nxs_resp_tojson(nxs_resp_t *, size_t *);
void		nxs_resp_release(nxs_resp_t *);

/*
 * Total match count (new; the reference has no such key).  nxs_resp_resultcount() and the
 * JSON "count" are the number of results RETURNED, at most `limit` (results.c:196,218).
 * A search whose params carry "total": true (bool, default false) also counts how many
 * docs matched: the number of results an unbounded limit would return, i.e. the
 * cardinality of the expression's doc set (get_expr_bitmap, search.c:118-174) -- 0 under a
 * ranking function that scores nothing (BM25 on an index with adl < 1, ranking.c:163-166).
 * It does not depend on the limit or otherwise on the ranking function, leaves out removed
 * docs, and belongs to the snapshot the batch's results came from.
 * nxs_resp_total() returns false, *total untouched, if the search did not ask; the JSON
 * then is what it always was, else it ends ...],"count":N,"total":M}.
 * Served by nxs_index_search, nxs_index_search_batch[_begin/_end] (any mix of asking and
 * non-asking batches in flight) and nxs_docshard_search_batch (the shards hold disjoint
 * docs: the sum of their totals).  REFUSED for now -- the whole batch fails with -1 and
 * NXS_ERR_INVALID "total is not available on a sharded batch" -- with a communicator
 * attached, in an emulated world of more than one rank, and by
 * nxs_docshard_search_batch_rank(): the totals would have to travel in the record and
 * candidate blocks whose layout all ranks agree on; that is a follow-up.
 * nxs_index_plan_batch() ignores the key.
 */
bool		nxs_resp_total(const nxs_resp_t *, uint64_t *total);

/*
 * Explanations (new; the reference has no such key).  A search whose params carry "explain": true (bool,
 * default false; with it false or absent nothing changes) also reports, for every returned doc, what each
 * token of the query's token list added to its score.  The token list is what the query RESOLVED to -- after
 * the filters, the fuzzy lookup and the expansion of prefix leaves; right to left, merged, unresolved tokens
 * left out, a term reached twice listed twice -- in the order the scores are added (run_query_logic,
 * search.c:236-270).  Every token whose term holds the doc contributes, also one that stands under a NOT or in
 * another OR branch: the expression only decides which docs are returned.  The contributions of the present
 * tokens, added in f32 in ascending token order starting from 0, ARE the returned score, bit for bit.
 *
 * nxs_resp_tokens():  m, the length of the token list; 0 if the search did not ask or matched nothing.
 * nxs_resp_token():   the bytes of the dictionary term token j resolved to (owned by the response,
 *                     NUL-terminated); false if j is out of range.
 * nxs_resp_explain(): result i (iteration order), token j: the term count of the doc and the float the token
 *                     added; false = absent (the doc does not hold the term), out of range, or not asked.
 *                     The out pointers may be NULL.
 * The JSON of an asking search: {"results":[{"doc_id":N,"score":X,"terms":[{"t":J,"tf":N,"score":X},...]},
 * ...],"count":K[,"total":M],"tokens":["term",...]} -- "terms" holds the present tokens in ascending J.
 *
 * The explanation belongs to the snapshot the results came from (a batch finished early because the files
 * moved is explained before the index follows them) and covers every limit and plan size.  Served by
 * nxs_index_search, nxs_index_search_batch[_begin/_end] (any mix of asking and non-asking batches in flight;
 * query-sharded: every rank explains the responses it holds from its own replica, no collective) and
 * nxs_docshard_search_batch (each row comes from the shard that holds the doc).  REFUSED -- -1 and
 * NXS_ERR_INVALID "explain is not available on a ranked doc-shard batch" -- by
 * nxs_docshard_search_batch_rank().  nxs_index_plan_batch() ignores the key.
 */
unsigned	nxs_resp_tokens(const nxs_resp_t *);
bool		nxs_resp_token(const nxs_resp_t *, unsigned j, const char **term, size_t *len);
bool		nxs_resp_explain(const nxs_resp_t *, unsigned i, unsigned j, float *score, uint32_t *tf);

/*
 * Spelling suggestions (new; the reference has no "did you mean" call).  For one raw token -- not a
 * query: the string goes through the index's filters as a query token does (normalizer / lowercase,
 * stop words, stemmer) and is then compared as it stands -- the ELIGIBLE terms are the dictionary
 * terms that
 *   - have a posting in a live doc of the current snapshot (df > 0: a term whose docs were all removed
 *     is not suggested, whatever its on-disk total says), and
 *   - lie within byte-wise Levenshtein distance "suggest_maxdist" (uint, 1 or 2, default 2) of the
 *     token (levdist, src/algo/levdist.c:67-150).
 * The result is the first min(k, matches) of them, k = "suggest_limit" (uint, 1..NXS_SUGGEST_MAX,
 * default 5), in the order distance ascending, df descending, term id ascending -- each with its
 * bytes, distance and df -- and `matches`, the exact number of eligible terms.  A value out of range
 * fails the call with NXS_ERR_INVALID and a message that names the key.  An exact hit (distance 0) is
 * eligible and comes first.  On an index with the stemmer filter the token is stemmed and the
 * suggestions are STEMS, as the dictionary holds them.  A string the filters drop (a stop word)
 * yields an empty list, matches 0 and nxs_sugg_dropped() true: not an error.
 *
 * This is not the set "fuzzymatch" draws from: that search takes the first term the BK-tree walk
 * reaches (bktree.c:219-275, idxterm.c:238-242) -- one member of the set, not the nearest and not
 * the most frequent -- never enters the subtree below a distance-63 child and goes by the on-disk
 * totals.  The term a fuzzy search resolves a token to is in the list whenever it has df > 0 and
 * matches <= k.
 *
 * The call re-syncs with the files as nxs_index_search does and is allowed while batches are in
 * flight (nxs_index_search_batch_begin), a batch whose fuzzy pass is still pending included: it
 * runs on a stream and workspace of its own and neither finishes nor reorders them -- unless the
 * files have moved, which finishes them first as any _begin would (their responses wait for _end).
 * It is local: with a communicator attached (nxs_index_shard) every rank answers its own calls, no
 * collective, and while batches are in flight from the snapshot they run on.  On a handle from
 * nxs_index_open_shard it fails with NXS_ERR_INVALID "suggest is not available on a doc shard" (a
 * shard's dictionary and df are collection-wide, its postings are not: a follow-up).
 *
 * nxs_index_suggest_batch: out[i] receives an object or NULL if token i failed (errs[i], may be
 * NULL); returns the number of failed tokens, or -1 if the batch could not run (nxs_get_error).
 * nxs_sugg_get: false if i >= nxs_sugg_count(); *term is owned by the object, NUL-terminated (any of
 * the out pointers may be NULL).  nxs_sugg_tojson (the caller frees, like nxs_resp_tojson):
 *   {"token":"<filtered token>","suggestions":[{"term":"...","distance":1,"df":12},...],"matches":7}
 * strings pass UTF-8 through; a double quote, a backslash and every byte below 0x20 (the last as a
 * six-character escape: backslash, u, 00 and two hex digits) are escaped.
 */
#define	NXS_SUGGEST_MAX		32
struct nxs_sugg;
typedef struct nxs_sugg nxs_sugg_t;

nxs_sugg_t *	nxs_index_suggest(nxs_index_t *, nxs_params_t *, const char *token, size_t len);
int		nxs_index_suggest_batch(nxs_index_t *, nxs_params_t *,
		    const char *const *tokens, size_t n,
		    nxs_sugg_t **out, nxs_err_t *errs);
unsigned	nxs_sugg_count(const nxs_sugg_t *);
uint64_t	nxs_sugg_matches(const nxs_sugg_t *);
bool		nxs_sugg_dropped(const nxs_sugg_t *);
bool		nxs_sugg_get(const nxs_sugg_t *, unsigned i, const char **term, size_t *len,
		    unsigned *distance, uint64_t *df);
char *		nxs_sugg_tojson(nxs_sugg_t *, size_t *);
void		nxs_sugg_release(nxs_sugg_t *);

/*
 * Prefix matching (new; the reference's lexer takes `*` for an ordinary byte of a free-form string,
 * scan.re:76, so `micro*` is looked up verbatim there).
 *
 * The ELIGIBLE terms of a non-empty prefix p are the dictionary terms that have a posting in a live doc of
 * the current snapshot (df > 0, the rule of the suggestions) and whose first len(p) bytes equal p; the term
 * equal to p is eligible.  Their ORDER is df descending, then term id ascending: a total order.  A prefix is
 * a fragment, not a word: it takes the normalizer / lowercase stage of the index's pipeline only -- no stop
 * words (`th*` must not vanish), no stemmer.  On an index with the stemmer filter the dictionary holds
 * STEMS, so the completions are stems.
 *
 * nxs_index_complete: the first min(k, matches) eligible terms of `prefix`, k = "complete_limit" (uint,
 * 1..NXS_SUGGEST_MAX, default 5; out of range: NXS_ERR_INVALID naming the key), as an nxs_sugg_t read
 * through the accessors above: nxs_sugg_get reports distance = len(term) - len(p), the pair's true
 * Levenshtein distance; nxs_sugg_matches is the exact number of eligible terms; nxs_sugg_dropped is false.
 * A prefix that is empty before or after normalisation is NXS_ERR_INVALID "empty prefix".
 * nxs_sugg_tojson of such an object:
 *   {"prefix":"<normalised prefix>","completions":[{"term":"...","df":12},...],"matches":7}
 * with the escaping rules above.  nxs_index_complete_batch: as nxs_index_suggest_batch.  Everything else is
 * nxs_index_suggest's: the call re-syncs with the files as a search does, is allowed while batches (or a
 * batch's pending fuzzy pass) are in flight and neither finishes nor reorders them, is local under a
 * communicator, and on a handle from nxs_index_open_shard fails with NXS_ERR_INVALID "complete is not
 * available on a doc shard".
 *
 * Prefix leaves in queries: "prefixmatch" (bool, default FALSE) and "prefix_limit" (uint, 1..32, default 8;
 * out of range: NXS_ERR_INVALID naming the key).  With prefixmatch false or absent nothing changes: `micro*`
 * is the free-form string it always was.  With it, a leaf that comes from a free-form (not a quoted) string
 * and ends in `*` with at least one byte in front of it is a prefix leaf: the star goes, the rest is
 * normalised to p, and the query behaves EXACTLY as the query in which that leaf is the sub-expression
 * (e1 OR e2 OR ... OR em), e1..em the first min(prefix_limit, matches) eligible terms of p in the order above,
 * each an already resolved term (no filters, no fuzzy lookup): the doc set, the token set and its order
 * (hence the float summation order and the ties), duplicates merged with the query's other tokens, and
 * "total".  m = 0 makes the leaf the empty set.  A prefix leaf is never fuzzy-matched; the other leaves are,
 * as always.  A lone `*` and a quoted "micro*" are ordinary leaves.  The expansions count towards the
 * existing limits (truth table up to 8 live tokens, the wide plan above 32, NXS_ERR_LIMIT beyond that).
 * Served by nxs_index_search, nxs_index_search_batch[_begin/_end] (any mix of batches in flight; the batch's
 * distinct prefixes are resolved by one blocking device pass in _begin), nxs_index_plan_batch and
 * query-sharded batches (the replicas hold the same dictionary and df: every rank derives the same
 * expansions).  The nxs_docshard_* searches refuse a batch that holds a prefix leaf: -1 and NXS_ERR_INVALID
 * "prefixmatch is not available on a doc shard".
 */
nxs_sugg_t *	nxs_index_complete(nxs_index_t *, nxs_params_t *, const char *prefix, size_t len);
int		nxs_index_complete_batch(nxs_index_t *, nxs_params_t *,
		    const char *const *prefixes, size_t n,
		    nxs_sugg_t **out, nxs_err_t *errs);

/*
 * Wildcard term matching (new; the reference's lexer takes `*` and `?` for ordinary bytes of a free-form
 * string, so `micro*ft` is looked up verbatim there).
 *
 * A PATTERN is a byte string: `*` matches any run of bytes, the empty run included; `?` matches exactly one
 * byte (byte-wise, as the Levenshtein distance and the prefixes here are); every other byte matches itself.
 * There are no escapes and no classes.  A term matches when the whole term matches the whole pattern.
 * Normalisation: the pattern is cut at its metacharacters, each literal piece takes the normalizer /
 * lowercase stage of the index's pipeline only (the rule of a prefix, for the same reason: a fragment is not
 * a word), the pieces are put back together and runs of `*` collapse to one.  A pattern that holds no literal
 * byte after normalisation (`*`, `??`, `*?*`) is not served: in a call it is NXS_ERR_INVALID "empty
 * pattern", in a query the leaf is the empty set, as a prefix that normalises to nothing is.  A normalised
 * pattern longer than NXS_WILD_MAXLEN (255) bytes is NXS_ERR_INVALID "wildcard pattern too long"; in a batch
 * that error belongs to the query (string) that holds the pattern -- errs[i] -- not to the batch.
 * The ELIGIBLE terms are the dictionary terms that have a posting in a live doc of the current snapshot
 * (df > 0, the rule of suggestions and completions) and match.  Their ORDER is df descending, then term id
 * ascending: a total order.  `matches` is the exact number of eligible terms, however large.
 *
 * nxs_index_wildcard: the first min(k, matches) eligible terms of `pattern`, k = "wildcard_limit" (uint,
 * 1..NXS_SUGGEST_MAX, default 5; out of range: NXS_ERR_INVALID naming the key), as an nxs_sugg_t:
 * nxs_sugg_get reports distance = len(term) - the number of literal bytes of the pattern; nxs_sugg_matches
 * is exact; nxs_sugg_dropped is false.  nxs_sugg_tojson of such an object:
 *   {"pattern":"<normalised pattern>","terms":[{"term":"...","df":12},...],"matches":7}
 * with the escaping rules above.  nxs_index_wildcard_batch: as nxs_index_suggest_batch.  Everything else is
 * nxs_index_complete's: the call re-syncs with the files, is allowed with batches or a pending fuzzy pass in
 * flight, is local under a communicator, and on a handle from nxs_index_open_shard fails with
 * NXS_ERR_INVALID "wildcard is not available on a doc shard".
 *
 * Wildcard leaves in queries: "wildcardmatch" (bool, default FALSE) and "wildcard_terms" (uint, 1..32,
 * default 8; out of range: NXS_ERR_INVALID naming the key).  With wildcardmatch false or absent nothing
 * changes: `*` and `?` stay ordinary bytes of a free-form string.  With it, a leaf that comes from a
 * free-form (never a quoted) string is a wildcard leaf when it holds a `*` or `?` and at least one other
 * byte.  One exception keeps "prefixmatch" as it is: with that flag set too, a literal followed by a single
 * trailing `*` and no other metacharacter is the prefix leaf it is today, with prefix_limit.  The query
 * behaves EXACTLY as the query in which the leaf is (e1 OR e2 OR ... OR em), e1..em the first
 * min(wildcard_terms, matches) eligible terms in the order above, each already resolved (no filters, no fuzzy
 * lookup): doc set, token set and order, ties, "total" and "explain" follow the rewritten query.  A wildcard
 * leaf is never fuzzy-matched; m = 0 makes it the empty set; the expansions count towards the existing token
 * limits.  Served by nxs_index_search, nxs_index_search_batch[_begin/_end] (the batch's distinct patterns are
 * resolved by one blocking device pass in _begin), nxs_index_plan_batch and query-sharded batches (the
 * replicas hold one dictionary and df).  The nxs_docshard_* searches refuse a batch that holds a wildcard
 * leaf: -1 and NXS_ERR_INVALID "wildcardmatch is not available on a doc shard".
 */
#define	NXS_WILD_MAXLEN		255
nxs_sugg_t *	nxs_index_wildcard(nxs_index_t *, nxs_params_t *, const char *pattern, size_t len);
int		nxs_index_wildcard_batch(nxs_index_t *, nxs_params_t *,
		    const char *const *patterns, size_t n,
		    nxs_sugg_t **out, nxs_err_t *errs);

/*
 * Similar documents (new; the reference has no "more like this" call, and no call that starts from a doc).
 *
 * TERM VECTOR.  For a live doc d of the current snapshot, a ranking function `algo` and mindf >= 1 the
 * ELIGIBLE terms are the dictionary terms t that have a posting in d, whose live df (the rule of the
 * suggestions) is at least mindf, and whose float w(t, d) = rank(t, d) under `algo` -- the float "explain"
 * reports for the pair -- is >= 0 (a negative rank adds nothing to any score, search.c:258).  That last rule
 * is defensive: the reference's rank() is negative only for tf <= 0 or an average doc length below 1 -- its
 * BM25 idf is log(1 + (N - df + 0.5) / (df + 0.5)) and its TF-IDF idf log(N / df) + 1 (ranking.c), never
 * negative, so a term in more than half the docs IS eligible -- and no posting of a live doc, hence no test,
 * reaches the w < 0 branch on either route.  Their ORDER is w descending as floats, then term id ascending: a total order.  `matches` is
 * the exact number of eligible terms.
 *
 * nxs_index_doc_terms: the first min(k, matches) eligible terms of `doc`, k = "docterms_limit" (uint,
 * 1..NXS_SUGGEST_MAX, default 5), mindf = "docterms_mindf" (uint >= 1, default 1; out of range:
 * NXS_ERR_INVALID naming the key), "algo" read as a search reads it (the impacts are materialised on demand,
 * as by a search), as an nxs_sugg_t: nxs_sugg_get reports the term's bytes, distance = the doc's term count
 * (tf) and df; nxs_sugg_score reports w (false on an object of the other calls and for i out of range);
 * nxs_sugg_matches is exact; nxs_sugg_dropped is false.  nxs_sugg_tojson of such an object:
 *   {"doc_id":7,"terms":[{"term":"...","tf":3,"df":12,"score":1.25},...],"matches":7}
 * the float as nxs_resp_tojson writes a score, strings with the escaping rules above.  A doc id that is not a
 * live doc of the snapshot -- never seen, or removed -- is NXS_ERR_MISSING "no such document"; in a batch
 * that is errs[i], and the call goes on.  nxs_index_doc_terms_batch: as nxs_index_suggest_batch.  Everything
 * else is nxs_index_complete's: the call re-syncs with the files, is allowed with batches or a pending fuzzy
 * pass in flight and neither finishes nor reorders them, is local under a communicator, and on a handle from
 * nxs_index_open_shard fails with NXS_ERR_INVALID "doc_terms is not available on a doc shard".
 *
 * nxs_index_similar: "similar_terms" (uint, 1..32, default 8), "similar_mindf" (uint >= 1, default 2: a term
 * that only d holds has the largest idf and finds nothing; out of range: NXS_ERR_INVALID naming the key),
 * "similar_self" (bool, default FALSE); "limit", "algo", "total" and "explain" as a search reads them;
 * "fuzzymatch", "prefixmatch" and "wildcardmatch" are ignored (every term is resolved already).  Let e1..em
 * be the first min(similar_terms, matches) eligible terms of d at mindf = similar_mindf.  With similar_self
 * the response is EXACTLY that of the query (e1 OR e2 OR ... OR em), each ei an already resolved term (no
 * filters, no lookup -- the rule of a prefix leaf): doc set, token set and order, float summation order, ties,
 * "total" and "explain" follow the rewritten query.  Without it (the default) the query runs at limit + 1,
 * the entry of d is removed if it is among the results, and the first `limit` are kept; d always matches when
 * m >= 1, so "total" is the rewritten query's minus 1, and with "explain" the removed result's row goes with
 * it.  m = 0 is an empty response with total 0, not an error.  limit + 1 must still be a valid limit
 * (NXS_ERR_INVALID "invalid limit").  A doc that is not live fails with NXS_ERR_MISSING as above; a doc shard
 * is refused with NXS_ERR_INVALID "similar is not available on a doc shard".  Under a communicator the call
 * behaves as nxs_index_search_batch of the rewritten queries (the replicas hold one dictionary, df and
 * postings: every rank derives the same expansions; "total" stays refused there), and the _batch form stands
 * to batches in flight as nxs_index_search_batch does.  The batch's docs are resolved by one blocking device
 * pass.
 */
nxs_sugg_t *	nxs_index_doc_terms(nxs_index_t *, nxs_params_t *, nxs_doc_id_t doc);
int		nxs_index_doc_terms_batch(nxs_index_t *, nxs_params_t *, const nxs_doc_id_t *docs, size_t n,
		    nxs_sugg_t **out, nxs_err_t *errs);
bool		nxs_sugg_score(const nxs_sugg_t *, unsigned i, float *score);
nxs_resp_t *	nxs_index_similar(nxs_index_t *, nxs_params_t *, nxs_doc_id_t doc);
int		nxs_index_similar_batch(nxs_index_t *, nxs_params_t *, const nxs_doc_id_t *docs, size_t n,
		    nxs_resp_t **resps, nxs_err_t *errs);

/*
 * Related terms (new; the reference has no call that starts from a result set): the dictionary terms that occur
 * in a query's matches -- facet counts, "refine your search", tag clouds.
 *
 * DOC SET.  For a query string and params let M be the doc set of the query's expression: exactly what "total"
 * counts -- live docs only, and empty under a ranking function that scores nothing.  The query is parsed,
 * filtered and resolved as nxs_index_search would with the same params: "fuzzymatch", "prefixmatch" /
 * "prefix_limit", "wildcardmatch" / "wildcard_terms" and "algo" are read as a search reads them; "limit", "total"
 * and "explain" are ignored.  n = |M|.
 *
 * COUNTS.  For a dictionary term t, c(t) = the number of docs of M that hold t -- doc membership: a doc with tf
 * 3 counts once --, df(t) = its live df (the rule of the suggestions).
 *
 * ELIGIBLE are the terms with c(t) >= "related_mincount" (uint >= 1, default 1), df(t) >= "related_mindf" (uint
 * >= 1, default 1) that are not a term of the query's resolved token list -- what nxs_resp_tokens would report:
 * tokens under a NOT and the expansions of prefix and wildcard leaves included.  "related_self" (bool, default
 * false) set to true lifts that exclusion.
 *
 * ORDER.  "related_order" (string, default "count"); both values give a total order:
 *   "count"  c descending, then term id ascending;
 *   "share"  s descending as floats, then term id ascending, s(t) = the f32 nearest to the fp64 quotient
 *            (double)c / (double)df.  c / df orders exactly as the lift (c / n) / (df / N) does, n and N being
 *            constants of the query.  s >= 0 always.
 * Any other string, or a uint out of range, fails the call with NXS_ERR_INVALID and a message that names the key.
 *
 * RESULT.  The first min(k, matches) eligible terms in that order, k = "related_limit" (uint,
 * 1..NXS_SUGGEST_MAX, default 5), as a fifth kind of nxs_sugg_t: nxs_sugg_get reports the term's bytes,
 * distance = c and df = the live df; nxs_sugg_score reports s, under either order; nxs_sugg_matches is the exact
 * number of eligible terms; nxs_sugg_dropped is false; nxs_sugg_docs reports n (false on an object of the other
 * calls).  nxs_sugg_tojson of such an object:
 *   {"query":"<the string as given>","docs":n,"terms":[{"term":"...","count":c,"df":df,"score":s},...],"matches":M}
 * the float as nxs_resp_tojson writes a score, strings with the escaping rules above.
 *
 * EDGE CASES.  n = 0, or a query that resolves to nothing: an empty list with docs 0 and matches 0, not an
 * error.  A query of more than 32 live tokens (a search's wide plan) is refused with NXS_ERR_LIMIT "related is
 * not available for a query of more than 32 terms"; a parse error is what a search reports for the string.  In a
 * batch both are errs[i], and the batch goes on.  nxs_index_related_batch: as nxs_index_suggest_batch.
 * Everything else is nxs_index_doc_terms': the call re-syncs with the files, is allowed with batches or a
 * pending fuzzy pass in flight and neither reorders them nor changes their responses (a batch whose second half
 * still waits for its fuzzy pass is sent on to the device first when this call's own tokens need that pass), is
 * local under a communicator, and on a handle from nxs_index_open_shard fails with NXS_ERR_INVALID
 * "related is not available on a doc shard".
 */
nxs_sugg_t *	nxs_index_related(nxs_index_t *, nxs_params_t *, const char *query, size_t len);
int		nxs_index_related_batch(nxs_index_t *, nxs_params_t *, const char *const *queries, size_t n,
		    nxs_sugg_t **out, nxs_err_t *errs);
bool		nxs_sugg_docs(const nxs_sugg_t *, uint64_t *docs);

/*
 * ---- search within a doc-id set (new) -------------------------------------------------
 *
 * nxs_index_search_docs ranks a caller's candidates: the docs of an access-control list, of an earlier result
 * list, of another index.  Raising "limit" and filtering afterwards is not the same thing: the reference's
 * comparator calls equal scores equal (result_entry_cmp), so which of several tied docs survive a capped heap
 * depends on the feed sequence, and taking docs out of that sequence changes the outcome.
 *
 * PARSING AND PARAMETERS.  Query i is parsed, filtered and resolved exactly as nxs_index_search would with the same
 * params: "limit", "algo", "fuzzymatch", "prefixmatch" / "prefix_limit", "wildcardmatch" / "wildcard_terms",
 * "total" and "explain" are read as a search reads them.
 *
 * THE SET.  Let R be the results of that query at an unbounded limit, as (doc, score) pairs; the scores are the
 * index's: N, df, adl and idf do not depend on the set.  Let S be the distinct ids of docs[i] that are live docs
 * of the snapshot.  Duplicates count once.  Ids never seen or removed are ignored silently: a stale
 * access-control list is normal, not an error.
 *
 * THE RESPONSE is exactly what the reference produces when nxs_resp_addresult is reached only for docs of S: R n S
 * is fed in descending doc id (results.c prepends, the build walks the list) into the reference's capped heap of
 * "limit" entries, then heap_sort runs; ties fall where that heap puts them.  A doc of S is in R when the
 * expression holds on its presence mask and at least one present token has a non-negative float
 * (search.c:251-258).  With "total": nxs_resp_total = |R n S|.  With "explain": as a search's.  An empty S,
 * n_docs[i] == 0 with docs[i] == NULL, or a query that resolves to nothing all give an empty response with
 * total 0.
 *
 * ERRORS.  n_docs[i] > NXS_DOCSET_MAX: NXS_ERR_LIMIT "doc set too large".  More than 32 live tokens (a search's
 * wide plan): NXS_ERR_LIMIT "search_docs is not available for a query of more than 32 terms".  A parse error is
 * what a search reports.  In a batch all three are errs[i], and the batch goes on.  On a handle from
 * nxs_index_open_shard: NXS_ERR_INVALID "search_docs is not available on a doc shard".
 *
 * SHARED SETS.  Two queries of a batch whose docs[i] pointer and n_docs[i] are both equal share one set: it is
 * sorted and resolved once (one access-control list across many queries).
 *
 * Everything else is nxs_index_related's: the call re-syncs with the files as a search does, is allowed with
 * batches or a pending fuzzy pass in flight and neither reorders them nor changes their responses, runs on a
 * stream and workspace of its own and is blocking, and is local under a communicator: no collective, and "total"
 * is served.  nxs_index_search_docs_batch returns the number of failed queries, or -1 if the batch as a whole
 * could not run.
 */
#define	NXS_DOCSET_MAX		(1u << 22)
nxs_resp_t *	nxs_index_search_docs(nxs_index_t *, nxs_params_t *, const char *query, size_t len,
		    const nxs_doc_id_t *docs, size_t n_docs);
int		nxs_index_search_docs_batch(nxs_index_t *, nxs_params_t *, const char *const *queries, size_t n,
		    const nxs_doc_id_t *const *docs, const size_t *n_docs, nxs_resp_t **resps, nxs_err_t *errs);

/*
 * ---- a query's matches listed by doc id (new) -----------------------------------------
 *
 * nxs_index_match_docs returns the doc set of a query itself, not a ranked and capped view of it: for export,
 * delete-by-query or re-index-by-query in the system that owns the documents, joins against another store, a stable
 * scroll through all hits, "search within these results".  Raising "limit" does none of this: a capped heap is
 * tie-order dependent and a deep page of it has no stable cursor.
 *
 * DOC SET.  M is the doc set of the query's expression: exactly what "total" counts and what nxs_index_related
 * calls M -- live docs only, and empty under a ranking function that scores nothing.  The query is parsed, filtered
 * and resolved as nxs_index_search would with the same params: "algo", "fuzzymatch", "prefixmatch" /
 * "prefix_limit", "wildcardmatch" / "wildcard_terms" are read as a search reads them; "limit", "total" and
 * "explain" are ignored.
 *
 * KEYS.  "match_limit" (uint, 1..NXS_MATCH_MAX, default 1000): the size of a page.  "match_from" (uint, default 0):
 * the smallest doc id admitted, inclusive -- no doc id has a special meaning.  A value out of range fails the call
 * with NXS_ERR_INVALID and a message that names the key.  nxs_index_match_docs_batch: from == NULL, or from[i]
 * replaces "match_from" for query i.
 *
 * RESULT.  The docs of M with id >= from, in ascending doc id, the first "match_limit" of them: nxs_docs_count of
 * them at nxs_docs_ids (owned by the object).  nxs_docs_total = |M|, whatever the cursor.  nxs_docs_next is true
 * exactly when a doc of M lies beyond the page; *from is then the last returned id + 1 (it cannot overflow: a larger
 * id exists), the cursor of the next page; false = the set is exhausted (*from is left alone).  Pages walked from
 * 0 until nxs_docs_next is false are disjoint, ascending, and their concatenation is M of a snapshot that does not
 * change meanwhile; after a refresh the walk goes on from its cursor over the new M.  The ids are ascending and
 * distinct, which is the one-pass fast path of nxs_index_search_docs: match_docs(q1) then search_docs(q2, ids) is
 * an exact search within the results of q1.  nxs_docs_tojson:
 *   {"query":"<the string as given>","docs":[1,5,9],"count":3,"total":120,"next":10}
 * "next" is absent when the set is exhausted; strings with the escaping rules of nxs_sugg_tojson.  The text is
 * malloc()ed: free() it.
 *
 * EDGE CASES.  A query that resolves to nothing, or an empty M: an empty page with total 0, not an error.  A
 * parse error is what a search reports for the string.  More than 32 live tokens (a search's wide plan):
 * NXS_ERR_LIMIT "match_docs is not available for a query of more than 32 terms".  In a batch both are errs[i], and
 * the batch goes on.  nxs_index_match_docs_batch returns the number of failed queries, or -1 if the batch as a
 * whole could not run.
 *
 * Everything else is nxs_index_related's: the call re-syncs with the files, is allowed with batches or a pending
 * fuzzy pass in flight and neither reorders them nor changes their responses, is blocking on a stream and
 * workspace of its own, is local under a communicator, and on a handle from nxs_index_open_shard fails with
 * NXS_ERR_INVALID "match_docs is not available on a doc shard" (the shards' pages would concatenate: a follow-up).
 */
#define	NXS_MATCH_MAX		(1u << 22)
struct nxs_docs;
typedef struct nxs_docs nxs_docs_t;

nxs_docs_t *	nxs_index_match_docs(nxs_index_t *, nxs_params_t *, const char *query, size_t len);
int		nxs_index_match_docs_batch(nxs_index_t *, nxs_params_t *, const char *const *queries, size_t n,
		    const nxs_doc_id_t *from /* NULL, or [n]: per-query cursors */, nxs_docs_t **out, nxs_err_t *errs);
size_t		nxs_docs_count(const nxs_docs_t *);
const nxs_doc_id_t *nxs_docs_ids(const nxs_docs_t *);		/* [count], ascending; owned by the object */
uint64_t	nxs_docs_total(const nxs_docs_t *);		/* |M|, whatever the cursor */
bool		nxs_docs_next(const nxs_docs_t *, nxs_doc_id_t *from);	/* true + cursor of the next page, false = exhausted */
char *		nxs_docs_tojson(nxs_docs_t *, size_t *);
void		nxs_docs_release(nxs_docs_t *);

/*
 * Batch entry point (new).  Runs `n` queries with one set of params as one
 * device batch.  resps[i] receives a response object or NULL if query i
 * failed (its code/message are then in errs[i]/the nxs_t error slot for the
 * last failure).  Returns the number of failed queries, or -1 if the batch as
 * a whole could not run (nxs_get_error() tells why).
 */
int		nxs_index_search_batch(nxs_index_t *, nxs_params_t *,
		    const char *const *queries, size_t n,
		    nxs_resp_t **resps, nxs_err_t *errs);

/*
 * The same, split for pipelining (new): _begin() parses, resolves and plans
 * the batch on the host (worker threads), queues it on the device and returns;
 * _end() waits for the OLDEST batch in flight and builds its responses.  Up to
 * NXS_BATCHES_INFLIGHT batches may be in flight, so the host prepares batch i+1
 * while the GPU runs batch i (two hide the host side of a top-10 batch; at the
 * default limit of 1000 a batch ends in milliseconds of heap replay on a nearly
 * idle chip, and three or four in flight fill it).  `queries` need not outlive _begin().  The index re-syncs with
 * the files (search.c:309-312) in every _begin: when they have moved while batches
 * are in flight, _begin finishes those first (their responses wait for _end).
 */
#define	NXS_BATCHES_INFLIGHT	4
int		nxs_index_search_batch_begin(nxs_index_t *, nxs_params_t *,
		    const char *const *queries, size_t n);
int		nxs_index_search_batch_end(nxs_index_t *, nxs_resp_t **resps,
		    nxs_err_t *errs);

/*
 * Query sharding over the GPUs of one node (new; the reference scales out with
 * independent worker processes, compose/nginx.conf:2).  One process per GPU,
 * each with a replica of the index (NXS_GPU_DEVICE selects the device at open).
 * Rank 0 calls nxs_shard_unique_id(), the application hands the
 * NXS_SHARD_UID_BYTES bytes to the other ranks, then EVERY rank calls
 * nxs_index_shard() (collective: it builds an RCCL communicator).  From then on
 * every rank passes the SAME batch to nxs_index_search_batch[_begin]; each
 * rank runs its contiguous slice, one RCCL all-gather of fixed-size per-query
 * records over xGMI reassembles the batch, and every rank receives all n
 * responses.  Applies to limit <= 8000 (NXSGPU_BIG_K: fixed-size records); larger
 * limits run replicated (every rank computes the whole batch).  nxs_index_search()
 * (one query) never shards.  Re-sync with a communicator attached: a rank that sees
 * the files move while batches are in flight says so in its record block; all ranks
 * read that at the batch's _end and finish their batches in flight + re-read the
 * files in their next _begin (the same one on every rank: two batches after the
 * change was noticed in a fully pipelined loop).  A rank that cannot do its share of a batch still contributes an
 * "aborted" block, so every rank fails that batch together and the next one is in
 * step -- only a rank that cannot reach the collective at all (device memory for
 * the staging buffer, a dead process) stalls the group, as with any collective.
 * nxs_index_shard(idx, 0, 1, NULL) detaches.
 */
#define	NXS_SHARD_UID_BYTES	128
int		nxs_shard_unique_id(nxs_t *, uint8_t *uid);
int		nxs_index_shard(nxs_index_t *, int rank, int world, const uint8_t *uid);
/*
 * nxs_index_shard_local(idx, true): like the reference's worker processes, which answer only their own
 * requests (compose/nginx.conf:2), a rank then materialises the responses of ITS slice only: after _end
 * resps[i] is NULL and errs[i] untouched for the queries other ranks own, and the return value counts the
 * own slice's failures -- O(n / world) host work per rank and batch.  nxs_index_shard_slice() tells which
 * part [*lo, *hi) of an n-query batch that is (the whole batch when the mode is off or nothing is attached).
 */
int		nxs_index_shard_local(nxs_index_t *, bool on);
void		nxs_index_shard_slice(const nxs_index_t *, size_t n, size_t *lo, size_t *hi);

/*
 * Front half of a batch only: parse + resolve (fuzzy misses on the device) +
 * compile into device plans (struct nxsgpu_query = nxsgpu_query_t of
 * nxs_gpu.h), for callers that keep the results on the device
 * (nxsgpu_search_dev).  plans[i].n_tokens == 0 when query i matches nothing
 * or failed (errs[i] then holds its code).  Returns #failed or -1.
 */
struct nxsgpu_query;
int		nxs_index_plan_batch(nxs_index_t *, nxs_params_t *,
		    const char *const *queries, size_t n,
		    struct nxsgpu_query *plans, nxs_err_t *errs);

/*
 * Opens an index straight from the two files (no basedir/params.db): the
 * entry used by the bench and tests for synthetic corpora.  `algo` is the
 * index default ("BM25" / "TF-IDF"); `lowercase` enables the ASCII part of
 * the reference's "normalizer" filter for query tokens.
 */
nxs_index_t *	nxs_index_open_files(nxs_t *, const char *terms_path,
		    const char *dtmap_path, const char *algo, bool lowercase);

/*
 * Doc-sharded mode (new): for collections beyond one GPU's
 * memory.  Shard s of S holds the docs of rank [D*s/S, D*(s+1)/S) in ascending
 * doc id, scored with collection-wide statistics; nxs_docshard_search_batch()
 * runs a batch on every shard (each on its own device, `device` < 0 = the
 * NXS_GPU_DEVICE default) and merges the shards' candidates through one more
 * exact heap replay: the responses equal those of the unsharded index, ties
 * included.  limit <= 8000, at most 32 query terms.  The shards' passes run concurrently (every
 * shard has its own device / streams).
 *
 * A shard serves a static snapshot until the collection is refreshed, explicitly,
 * between batches: nxs_docshard_refresh() (all shards of the process, as passed to
 * nxs_docshard_search_batch) or nxs_docshard_refresh_rank() (collective, one process
 * per shard).  Every shard consumes the files up to ONE snapshot; appended docs go
 * to the last shard, a removal to the shard that holds the doc, new terms to every
 * dictionary; every shard's impacts are recomputed once with the collection-wide df.
 * A re-used or out-of-order doc id, or replaced files, rebuild every shard's slice.
 * Returns 1: the collection serves the new snapshot; 0: nothing had moved; -1: error
 * (nxs_get_error; the rank form: the same value on every rank).  A failure after
 * some shard's device state changed marks the collection inconsistent: searches
 * fail with NXS_ERR_FATAL until a refresh succeeds.
 *
 * One process per shard (one GPU each): rank r opens shard r of W, attaches a
 * communicator of W ranks (nxs_index_shard), joins the collection
 * (nxs_docshard_attach: all-gather + sum of the shards' df, collective) and
 * then every rank calls nxs_docshard_search_batch_rank() with the SAME batch:
 * each runs its shard, ONE all-gather of the ranks' candidate blocks, every
 * rank merges and holds all responses.
 */
nxs_index_t *	nxs_index_open_shard(nxs_t *, const char *terms_path,
		    const char *dtmap_path, const char *algo, bool lowercase,
		    unsigned shard, unsigned n_shards, int device);
int		nxs_docshard_search_batch(nxs_index_t *const *shards, unsigned n_shards,
		    nxs_params_t *, const char *const *queries, size_t n,
		    nxs_resp_t **resps, nxs_err_t *errs);
int		nxs_docshard_attach(nxs_index_t *shard);
int		nxs_docshard_search_batch_rank(nxs_index_t *shard, nxs_params_t *,
		    const char *const *queries, size_t n,
		    nxs_resp_t **resps, nxs_err_t *errs);
int		nxs_docshard_refresh(nxs_index_t *const *shards, unsigned n_shards);
int		nxs_docshard_refresh_rank(nxs_index_t *shard);

/* (test hooks and the bench's accessors -- nxs_index_host_profile, nxs_index_device, nxs_test_* -- are
 * not part of this ABI: nxsearch_amd/csrc/nxs_hooks.h, builds with -DNXS_TEST_HOOKS only) */

#ifdef __cplusplus
}
#endif
#endif
