/*
 * nxs_api_int.h -- what crosses the units of the public API's host side.  One unit per subsystem:
 *
 *   nxs_api.c       instance and error slot, index open / close
 *   nxs_pool.c      host worker pool
 *   nxs_params.c    nxs_params_t, the JSON scanner, the parameters of a search
 *   nxs_resp.c      response object: slab, accessors, JSON, explanations
 *   nxs_plan.c      plan cache and the front half of a batch (parse, lookups, prefixes, misses, compile)
 *   nxs_batch.c     begin / end, the late second half, exact fix-up and its protocol, query sharding
 *   nxs_lookup.c    nxs_sugg_t, suggest, complete, wildcard, doc_terms, related
 *   nxs_searchdocs.c  search within a caller's doc-id set (search_docs)
 *   nxs_matchdocs.c   a query's matches listed by doc id (match_docs), nxs_docs_t
 *   nxs_docshard.c  doc-sharded collections: search, attach, refresh
 *   nxs_hooks.c     the test hooks that reach no static
 *
 * A function used inside its unit only is static there, and a test hook that reaches a static lives in
 * that static's unit.  Nothing declared here is exported.
 */
#ifndef NXS_API_INT_H
#define NXS_API_INT_H

#include <string.h>
#include <time.h>

#include "nxs_impl.h"
#include "nxs_related.h"

#pragma GCC visibility push(hidden)

/* resps[i] = NULL, errs[i] = success: how every batch call starts (ptrs: [n] object pointers; errs may be NULL) */
static inline void
outs_clear(void *ptrs, nxs_err_t *errs, size_t n)
{
	if (n) {
		memset(ptrs, 0, n * sizeof(void *));
	}
	for (size_t i = 0; errs && i < n; i++) {
		errs[i] = NXS_ERR_SUCCESS;
	}
}

/* ---- nxs_pool.c ----------------------------------------------------------------------- */

typedef void (*pool_fn_t)(void *arg, size_t lo, size_t hi);

struct nxs_pool *nxs_pool_get(nxs_t *);
void	pool_run(struct nxs_pool *, pool_fn_t fn, void *arg, size_t n, size_t chunk);
void	pool_destroy(struct nxs_pool *);
void	api_parallel(void *ctx, nxsgpu_body_t body, void *arg, size_t n, size_t chunk);

/* ---- nxs_params.c --------------------------------------------------------------------- */

typedef struct {
	uint64_t	limit;
	int		algo;
	bool		fuzzymatch;
	bool		total;		/* "total": also count the matches (nxs_resp_total) */
	bool		prefixmatch;	/* "prefixmatch": a free-form leaf `term*` stands for its best completions */
	unsigned	prefix_limit;	/* "prefix_limit": how many of them (1..NXS_PREFIX_MAX, default 8) */
	bool		wildcardmatch;	/* "wildcardmatch": a free-form leaf with a `*` or `?` stands for its best matching terms */
	unsigned	wildcard_terms;	/* "wildcard_terms": how many of them (1..NXS_PREFIX_MAX, default 8) */
	bool		explain;	/* "explain": per result and token the term count and the score contribution */
	/* nxs_index_similar only */
	unsigned	similar_terms;	/* "similar_terms": expansions of the source doc (1..NXS_PREFIX_MAX, default 8) */
	unsigned	similar_mindf;	/* "similar_mindf": the df floor of an expansion (>= 1, default 2) */
	bool		similar_self;	/* "similar_self": the source doc stays among the results */
} search_params_t;

int	get_ranking_func_id(const char *name);
int	get_search_params(nxs_index_t *, nxs_params_t *, search_params_t *);

/* nxs_index_related's own keys (the query is read with a search's: search_params_t) */
typedef struct {
	unsigned	k;		/* "related_limit": terms returned (1..NXS_SUGGEST_MAX, default 5) */
	int		order;		/* "related_order": NXS_RT_COUNT ("count", the default) / NXS_RT_SHARE ("share") */
	unsigned	mindf;		/* "related_mindf": the df floor (>= 1, default 1) */
	unsigned	mincount;	/* "related_mincount": the floor of c (>= 1, default 1) */
	bool		self;		/* "related_self": the query's own terms stay eligible */
} related_params_t;

int	get_related_params(nxs_t *, const nxs_params_t *, related_params_t *);

/* nxs_index_match_docs' own keys (the query is read with a search's: search_params_t) */
typedef struct {
	unsigned	limit;		/* "match_limit": ids per page (1..NXS_MATCH_MAX, default 1000) */
	uint64_t	from;		/* "match_from": the smallest doc id admitted (default 0) */
} match_params_t;

int	get_match_params(nxs_t *, const nxs_params_t *, match_params_t *);

/* ---- nxs_resp.c ----------------------------------------------------------------------- */

struct resp_slab {
	size_t		refs;
	void *		ex;		/* the batch's explanations (explain_attach), or NULL: one block, freed with the slab */
};

struct nxs_resp {
	nxs_doc_id_t *	ids;
	float *		scores;
	unsigned	count;
	unsigned	iter;
	struct resp_slab *slab;		/* NULL: ids/scores are this response's own */
	bool		has_total;	/* the search asked for the total match count */
	uint64_t	total;
	/* "explain" (all in the slab's explain block; n_tok == 0: not asked, or nothing matched) */
	unsigned	n_tok;		/* tokens of the query's token list */
	const char *const *tok;		/* [n_tok] the dictionary terms they resolved to, NUL-terminated */
	const uint32_t *tok_len;	/* [n_tok] */
	const uint32_t *ex_tf;		/* [count][n_tok] term count of (result, token), 0 = absent */
	const float *	ex_imp;		/* [count][n_tok] what the token added to the result's score */
	bool		explained;	/* the search asked (the JSON then carries "tokens", be it empty) */
};

typedef struct {
	struct resp_slab *slab;
	nxs_resp_t *	resps;		/* [n] */
	nxs_doc_id_t *	ids;		/* [total] */
	float *		scores;		/* [total] */
	size_t		used;
} slab_builder_t;

int	slab_begin(slab_builder_t *, size_t n, size_t total);
void	slab_free(struct resp_slab *);
size_t	json_str(char *out, const char *s, size_t n);
size_t	fmt_real(char *out, double v);		/* a JSON real as nxs_resp_tojson writes a score; out: room for 40 bytes */

/* response i of the slab: `count` results to be filled in by the caller (per query: inline in its callers' units) */
static inline nxs_resp_t *
slab_resp(slab_builder_t *b, size_t i, unsigned count)
{
	nxs_resp_t *r = &b->resps[i];

	r->ids = b->ids + b->used;
	r->scores = b->scores + b->used;
	r->count = count;
	r->iter = 0;
	r->slab = b->slab;
	r->has_total = false;
	r->total = 0;
	r->n_tok = 0;
	r->tok = NULL;
	r->tok_len = NULL;
	r->ex_tf = NULL;
	r->ex_imp = NULL;
	r->explained = false;
	b->used += count;
	b->slab->refs++;
	return r;
}

/* one response to explain: its query's token list as the device saw it (nxsgpu_query_t::term_id) */
typedef struct {
	nxs_resp_t *	r;
	uint32_t	n_tok;
	const uint32_t *term_ids;
} ex_item_t;

/* the token list the device saw for a planned query (NULL plan: nothing to explain) */
static inline void
ex_item_of(ex_item_t *it, nxs_resp_t *r, const qprep_t *q)
{
	it->r = r;
	it->n_tok = q->wide ? q->wplan.n_tokens : q->plan.n_tokens;
	it->term_ids = q->wide ? q->wplan.term_id : q->plan.term_id;
}

int	explain_attach(nxs_index_t *const *shards, unsigned n_shards, int algo, const ex_item_t *items,
	    size_t n_items, struct resp_slab *slab);

/* ---- nxs_plan.c ----------------------------------------------------------------------- */

/* the tokens of a batch that missed the dictionary, as one byte string (tokenizer.c:177-180) */
typedef struct {
	uint32_t *	q, *t, *off, *ids;	/* [n]: query, token index, byte offset, winner */
	uint8_t *	bytes;
	size_t		n;
} fz_set_t;

/*
 * tokenizer.c:177-180 resolves a miss where it meets it; here a batch's misses are one device pass, and
 * _begin does not wait for it: it returns once the pass is queued, and the batch's second half runs
 * when the host comes by again (late_finish) -- the pass has had the caller's work on the previous
 * responses and the next batch's parse to finish in.  What the second half needs is kept here.
 */
struct late_half {
	search_params_t	sp;
	fz_set_t	fz;
	int		slot;		/* nxsgpu_fuzzy_begin's */
	bool		collected;	/* the pass is over, fz.ids hold the winners */
	char *		qbuf;		/* the strings still to compile (the caller's may be gone by then) */
	const char **	queries;	/* [hi - lo]: into qbuf; NULL = nothing left to do for that query */
};

void	plan_cache_destroy(struct plan_cache *);
int	plan_front(nxs_index_t *, const search_params_t *, const char *const *queries, const nxs_doc_id_t *docs, size_t n,
	    qprep_t *prep, fz_set_t *fz);
void	plan_back(nxs_index_t *, const search_params_t *, const char *const *queries, size_t n, qprep_t *prep,
	    const fz_set_t *fz);
int	plan_batch(nxs_index_t *, const search_params_t *, const char *const *queries, const nxs_doc_id_t *docs, size_t n,
	    qprep_t *prep);
void	fz_set_free(fz_set_t *);
struct late_half *late_make(const search_params_t *, fz_set_t *fz, const char *const *queries, size_t n,
	    const qprep_t *prep);
void	late_free(struct late_half *);

/* ---- nxs_batch.c ---------------------------------------------------------------------- */

static inline double
now_s(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

nxs_pend_t *pend_oldest(nxs_index_t *);
int	resync_before_batch(nxs_index_t *);
int	late_finish(nxs_index_t *);
void	index_drain(nxs_index_t *);

/* ---- nxs_lookup.c ---------------------------------------------------------------------- */

/* how every blocking side call begins (`what` names it in the refusal on a doc shard; bk: it reads the BK image):
 * refusals, the batch bound, the re-sync with the files.  0 / -1 with the error declared */
int	lookup_enter(nxs_index_t *, const char *what, size_t n, bool bk);

/* the rows nxsgpu_doc_terms fills for n docs at k terms each */
typedef struct {
	uint32_t	*ids, *tf, *df;	/* [n * k] */
	float *		w;		/* [n * k] */
	uint32_t	*counts, *matches;	/* [n] */
	uint8_t *	found;		/* [n] 1 = a live doc of the snapshot */
} docterms_rows_t;

/* the term vectors of docs[0 .. n): allocates the rows, runs the device pass, and clears `found` for a doc that
 * has been removed (it keeps its ordinal; the host's doc table knows).  0, or -1 with the error declared and
 * nothing left to free */
int	docterms_rows(nxs_index_t *, int algo, const nxs_doc_id_t *docs, size_t n, unsigned mindf, unsigned k,
	    docterms_rows_t *);
void	docterms_rows_free(docterms_rows_t *);

#pragma GCC visibility pop

#endif
