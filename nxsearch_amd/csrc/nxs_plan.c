/*
 * nxs_plan.c -- the front half of a batch: the plan cache, parse + dictionary
 * lookups + compile over the worker pool, the batch's prefix leaves and fuzzy
 * misses (one device pass each), and what a batch whose fuzzy pass is left
 * running keeps for its second half.
 *   token resolution      src/core/tokenizer.c:160-199 (exact, else fuzzy)
 */
#include <stdlib.h>
#include <string.h>

#include "nxs_api_int.h"

/*
 * Plan cache.  The reference builds a query_t per call (construct_query, search.c:176-208);
 * what that yields for a given query string -- tokens, their term ids, the boolean program --
 * depends only on the string, the `fuzzymatch` flag and the index's dictionary, so the
 * compiled plan of a string is kept until the index changes (any refresh clears the cache:
 * new terms change lookups and fuzzy winners).  A server's head queries then cost a hash
 * lookup and a 424-byte copy instead of lex + parse + resolve + compile (C2: planning was
 * 60 % of a 1024-query step).  Lookups run on the worker threads (read-only); the batch's
 * misses are inserted by the caller's thread afterwards.  Only plans that fit
 * nxsgpu_query_t and queries without errors are kept.  NXS_PLAN_CACHE=0 turns it off.
 * Under "prefixmatch" a string that holds a `*` bypasses the cache: what a prefix leaf stands for depends
 * on prefix_limit and on the df of the moment, and the same string means something else with the flag off.
 * The same holds for a string with a `*` or `?` under "wildcardmatch".
 */
typedef struct {
	uint64_t	h;
	char *		key;		/* NULL = empty slot */
	uint32_t	klen;
	uint8_t		fuzzy, empty;
	nxsgpu_query_t	plan;
} pc_ent_t;

struct plan_cache {
	pc_ent_t *	e;
	size_t		cap, n;		/* cap: a power of two */
	uint64_t	gen;		/* refreshes of the index when the entries were made */
	bool		off;
};

#define	PLAN_CACHE_CAP	(1u << 15)

static uint64_t
pc_hash(const char *s, size_t n, bool fuzzy)
{
	uint64_t h = 1469598103934665603ull ^ (fuzzy ? 0x9e3779b97f4a7c15ull : 0);

	for (size_t i = 0; i < n; i++) {
		h = (h ^ (uint8_t)s[i]) * 1099511628211ull;
	}
	return h ? h : 1;
}

static void
plan_cache_clear(struct plan_cache *pc)
{
	for (size_t i = 0; pc && pc->e && i < pc->cap; i++) {
		free(pc->e[i].key);
		pc->e[i].key = NULL;
	}
	if (pc) {
		pc->n = 0;
	}
}

void
plan_cache_destroy(struct plan_cache *pc)
{
	plan_cache_clear(pc);
	if (pc) {
		free(pc->e);
		free(pc);
	}
}

/* the cache of the index, valid for its current snapshot (NULL: off / out of memory) */
static struct plan_cache *
plan_cache_get(nxs_index_t *idx)
{
	/* (the dictionary can move without either refresh counter moving -- a refresh whose device half fails
	 * after sync_terms has consumed new terms --: what a lookup yields depends on the terms consumed) */
	const uint64_t gen = idx->n_incremental + idx->n_rebuilds + ((uint64_t)idx->last_id << 20);
	struct plan_cache *pc = idx->pcache;

	if (!pc) {
		const char *e = getenv("NXS_PLAN_CACHE");

		if ((pc = calloc(1, sizeof(*pc))) == NULL) {
			return NULL;
		}
		pc->off = e && atoi(e) == 0;
		pc->cap = PLAN_CACHE_CAP;
		if (!pc->off && (pc->e = calloc(pc->cap, sizeof(pc_ent_t))) == NULL) {
			pc->off = true;
		}
		pc->gen = gen;
		idx->pcache = pc;
	}
	if (pc->off) {
		return NULL;
	}
	if (pc->gen != gen || pc->n >= pc->cap / 2) {
		/* (half full: start over -- plan_cache_put refuses inserts from there on, so without this the table
		 * would stay frozen at its first 16 384 strings) */
		plan_cache_clear(pc);
		pc->gen = gen;
	}
	return pc;
}

void
nxs_plan_cache_switch(nxs_index_t *idx, int on)
{
	(void)plan_cache_get(idx);
	if (idx->pcache) {
		plan_cache_clear(idx->pcache);
		idx->pcache->off = !on;
		if (on && !idx->pcache->e && (idx->pcache->e = calloc(idx->pcache->cap, sizeof(pc_ent_t))) == NULL) {
			idx->pcache->off = true;
		}
	}
}

static const pc_ent_t *
plan_cache_find(const struct plan_cache *pc, const char *q, size_t n, bool fuzzy)
{
	const uint64_t h = pc_hash(q, n, fuzzy);

	for (size_t i = h & (pc->cap - 1); pc->e[i].key; i = (i + 1) & (pc->cap - 1)) {
		const pc_ent_t *e = &pc->e[i];
		if (e->h == h && e->klen == n && e->fuzzy == (uint8_t)fuzzy && memcmp(e->key, q, n) == 0) {
			return e;
		}
	}
	return NULL;
}

static void
plan_cache_put(struct plan_cache *pc, const char *q, size_t n, bool fuzzy, const qprep_t *p)
{
	const uint64_t h = pc_hash(q, n, fuzzy);
	size_t i = h & (pc->cap - 1);

	if (pc->n >= pc->cap / 2 || n > 4096) {
		return;
	}
	for (; pc->e[i].key; i = (i + 1) & (pc->cap - 1)) {
		if (pc->e[i].h == h && pc->e[i].klen == n && pc->e[i].fuzzy == (uint8_t)fuzzy &&
		    memcmp(pc->e[i].key, q, n) == 0) {
			return;		/* (twice in one batch) */
		}
	}
	if ((pc->e[i].key = malloc(n + 1)) == NULL) {
		return;
	}
	memcpy(pc->e[i].key, q, n);
	pc->e[i].key[n] = 0;
	pc->e[i].h = h;
	pc->e[i].klen = (uint32_t)n;
	pc->e[i].fuzzy = (uint8_t)fuzzy;
	pc->e[i].empty = (uint8_t)p->empty;
	pc->e[i].plan = p->plan;
	pc->n++;
}

/*
 * Front half of a batch: parse, build the token sets, resolve (exact on the
 * host, misses through one device BK-tree pass), compile the device plans.
 * prep[i].errcode / .empty tell how query i ended.  Parsing + lookups and the
 * compilation are spread over the instance's worker pool.
 */
typedef struct {
	const nxs_index_t *	idx;
	const search_params_t *	sp;
	const char *const *	queries;	/* or NULL: ... */
	const nxs_doc_id_t *	docs;		/* ... the batch is nxs_index_similar's, query i is doc i's leaf */
	qprep_t *		prep;
	const struct plan_cache *pc;	/* read-only while the workers run */
} plan_job_t;

static void
plan_parse_chunk(void *arg, size_t lo, size_t hi)
{
	const plan_job_t *j = arg;

	for (size_t i = lo; i < hi; i++) {
		qprep_t *q = &j->prep[i];

		if (j->docs) {
			nxs_query_prepare_doc(j->docs[i], q);
			if (q->errcode) {
				nxs_query_release_scratch(q);
				q->compiled = true;
			}
			continue;
		}
		if (j->pc && !(j->sp->prefixmatch && strchr(j->queries[i], '*')) &&
		    !(j->sp->wildcardmatch && strpbrk(j->queries[i], "*?"))) {
			const pc_ent_t *e = plan_cache_find(j->pc, j->queries[i], strlen(j->queries[i]), j->sp->fuzzymatch);
			if (e) {
				memset(q, 0, sizeof(*q));
				q->plan = e->plan;
				q->empty = e->empty != 0;
				q->cached = true;
				continue;
			}
		}
		nxs_query_prepare_wc(j->idx, j->queries[i], j->sp->prefixmatch, j->sp->wildcardmatch, q);
		if (q->errcode) {
			nxs_query_release_scratch(q);	/* (what the second pass would do for it) */
			q->compiled = true;
			continue;
		}
		/* idxterm_lookup for every token (tokenizer.c:171-176) */
		bool miss = false;
		for (size_t k = 0; k < q->n_tokens; k++) {
			qtok_t *t = &q->tokens[k];
			t->term_id = nxs_term_lookup(j->idx, (const uint8_t *)t->value, t->len);
			miss = miss || !t->term_id;
		}
		/* nothing of this query waits for the fuzzy search: compile it here and now -- a batch without
		 * misses (or with fuzzymatch off) is ONE run over the worker threads, not two */
		/* (a query with prefix leaves waits for the batch's completion pass: plan_prefixes) */
		if ((!miss || !j->sp->fuzzymatch) && !q->n_pfx) {
			(void)nxs_query_compile(q);
			nxs_query_release_scratch(q);
			q->compiled = true;
		}
	}
}

static void
plan_compile_chunk(void *arg, size_t lo, size_t hi)
{
	const plan_job_t *j = arg;

	for (size_t i = lo; i < hi; i++) {
		if (j->prep[i].cached || j->prep[i].compiled) {
			continue;
		}
		if (!j->prep[i].errcode) {
			(void)nxs_query_compile(&j->prep[i]);
		}
		/* the parse and the token list have done their job: freed here, on the
		 * worker, not on the caller's critical path */
		nxs_query_release_scratch(&j->prep[i]);
	}
}

void
fz_set_free(fz_set_t *fz)
{
	free(fz->q);
	free(fz->t);
	free(fz->off);
	free(fz->ids);
	free(fz->bytes);
	memset(fz, 0, sizeof(*fz));
}

typedef struct { const char *val; size_t len; uint32_t q, k, slot; } pfx_ref_t;

static int
pfx_ref_cmp(const void *a, const void *b)
{
	const pfx_ref_t *x = a, *y = b;

	if (x->len != y->len) {
		return x->len < y->len ? -1 : 1;
	}
	return memcmp(x->val, y->val, x->len);
}

/*
 * The prefix and wildcard leaves of a batch.  Per kind, the batch's distinct strings are resolved by ONE
 * blocking device pass -- nxsgpu_complete with k = prefix_limit, nxsgpu_wildcard with k = wildcard_terms
 * (plan_resolve) -- then each leaf's expansions are spliced into its query's program and token list
 * (nxs_query_splice), and a query that waits for nothing else is compiled.  A batch without such a leaf
 * makes no call.
 */
static int
plan_resolve(nxs_index_t *idx, size_t n, qprep_t *prep, int kind, unsigned k)
{
	nxs_t *nxs = idx->nxs;
	const char *what = kind == QPFX_WILD ? "wildcard" : "complete";
	size_t n_ref = 0, nd = 0, blen = 0, r = 0;
	pfx_ref_t *ref = NULL;
	uint8_t *bytes = NULL;
	uint32_t *off = NULL, *ids = NULL, *df = NULL, *counts = NULL, *matches = NULL;
	int ret = -1;

	for (size_t i = 0; i < n; i++) {
		for (size_t j = 0; !prep[i].errcode && j < prep[i].n_pfx; j++) {
			n_ref += prep[i].pfx[j].kind == kind;
		}
	}
	if (!n_ref) {
		return 0;
	}
	/* (a shard's postings are its own: the df the order rests on would be the shard's; include/nxs.h) */
	if (idx->n_shards) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "%s is not available on a doc shard",
		    kind == QPFX_WILD ? "wildcardmatch" : "prefixmatch");
		return -1;
	}
	if ((ref = malloc(n_ref * sizeof(*ref))) == NULL) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		return -1;
	}
	for (size_t i = 0; i < n; i++) {
		for (size_t j = 0; !prep[i].errcode && j < prep[i].n_pfx; j++) {
			if (prep[i].pfx[j].kind == kind) {
				ref[r++] = (pfx_ref_t){ prep[i].pfx[j].val, prep[i].pfx[j].len, (uint32_t)i, (uint32_t)j, 0 };
			}
		}
	}
	qsort(ref, n_ref, sizeof(*ref), pfx_ref_cmp);
	for (r = 0; r < n_ref; r++) {
		if (r == 0 || pfx_ref_cmp(&ref[r - 1], &ref[r]) != 0) {
			nd++;
			blen += ref[r].len;
		}
		ref[r].slot = (uint32_t)(nd - 1);
	}
	bytes = malloc(blen + 16);
	off = malloc((nd + 1) * sizeof(*off));
	ids = malloc(nd * k * sizeof(*ids));
	df = malloc(nd * k * sizeof(*df));
	counts = malloc(nd * sizeof(*counts));
	matches = malloc(nd * sizeof(*matches));
	if (!bytes || !off || !ids || !df || !counts || !matches || blen > UINT32_MAX / 2) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	blen = 0;
	for (r = 0; r < n_ref; r++) {
		if (r == 0 || ref[r].slot != ref[r - 1].slot) {
			off[ref[r].slot] = (uint32_t)blen;
			memcpy(bytes + blen, ref[r].val, ref[r].len);
			blen += ref[r].len;
		}
	}
	off[nd] = (uint32_t)blen;
	/* new terms reach the BK image first (as nxs_index_suggest: a batch whose fuzzy pass is still on the
	 * device reads the image, so that pass is waited for before the image is replaced) */
	if (idx->bk_upto != idx->last_id || idx->bk_flags_stale) {
		(void)late_finish(idx);
		if (nxs_index_bk_sync(idx) == -1) {
			goto out;
		}
	}
	if ((kind == QPFX_WILD ? nxsgpu_wildcard : nxsgpu_complete)(idx->dev, bytes, off, (uint32_t)nd, k, ids, df,
	    counts, matches) != 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "device %s pass failed: %s", what, nxsgpu_last_error());
		goto out;
	}
	for (r = 0; r < n_ref; r++) {
		qpfx_t *px = &prep[ref[r].q].pfx[ref[r].k];
		const uint32_t *row = ids + (size_t)ref[r].slot * k;

		px->n = counts[ref[r].slot] <= k ? counts[ref[r].slot] : k;
		for (uint32_t e = 0; e < px->n; e++) {
			if (row[e] < 1 || row[e] > idx->last_id) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "the device named an unknown term for a %s",
				    kind == QPFX_WILD ? "pattern" : "prefix");
				goto out;
			}
			px->ids[e] = row[e];
			px->tval[e] = idx->terms[row[e]].val;
			px->tlen[e] = idx->terms[row[e]].len;
		}
	}
	ret = 0;
out:
	free(ref);
	free(bytes);
	free(off);
	free(ids);
	free(df);
	free(counts);
	free(matches);
	return ret;
}

/*
 * The doc leaves of a batch (nxs_index_similar: every query is one): the batch's docs through ONE blocking
 * nxsgpu_doc_terms pass with k = similar_terms and mindf = similar_mindf (the device answers a doc given twice
 * once; docterms_rows, nxs_lookup.c).  A doc that is not live fails its query with NXS_ERR_MISSING.  (A doc
 * shard never gets here: nxs_index_similar_batch refuses it.)
 */
static int
plan_resolve_docs(nxs_index_t *idx, const search_params_t *sp, size_t n, qprep_t *prep)
{
	const unsigned k = sp->similar_terms;
	size_t nd = 0, r = 0;
	uint64_t *docs;
	docterms_rows_t rows;
	int ret = -1;

	for (size_t i = 0; i < n; i++) {
		nd += !prep[i].errcode && prep[i].n_pfx == 1 && prep[i].pfx[0].kind == QPFX_DOC;
	}
	if (!nd) {
		return 0;
	}
	if ((docs = malloc(nd * sizeof(*docs))) == NULL) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
		return -1;
	}
	for (size_t i = 0; i < n; i++) {
		if (!prep[i].errcode && prep[i].n_pfx == 1 && prep[i].pfx[0].kind == QPFX_DOC) {
			docs[r++] = strtoull(prep[i].pfx[0].val, NULL, 10);
		}
	}
	if (docterms_rows(idx, sp->algo, docs, nd, sp->similar_mindf, k, &rows) == -1) {
		free(docs);
		return -1;
	}
	r = 0;
	for (size_t i = 0; i < n; i++) {
		qpfx_t *px;
		const uint32_t *row;

		if (prep[i].errcode || prep[i].n_pfx != 1 || prep[i].pfx[0].kind != QPFX_DOC) {
			continue;
		}
		px = &prep[i].pfx[0];
		row = rows.ids + r * k;
		if (!rows.found[r]) {
			prep[i].errcode = NXS_ERR_MISSING;
			prep[i].errmsg = strdup("no such document");
			r++;
			continue;
		}
		px->n = rows.counts[r] <= k ? rows.counts[r] : k;
		for (uint32_t e = 0; e < px->n; e++) {
			if (row[e] < 1 || row[e] > idx->last_id) {
				nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "the device named an unknown term for a doc");
				goto out;
			}
			px->ids[e] = row[e];
			px->tval[e] = idx->terms[row[e]].val;
			px->tlen[e] = idx->terms[row[e]].len;
		}
		r++;
	}
	ret = 0;
out:
	free(docs);
	docterms_rows_free(&rows);
	return ret;
}

static int
plan_prefixes(nxs_index_t *idx, const search_params_t *sp, bool docs, size_t n, qprep_t *prep)
{
	if (docs ? plan_resolve_docs(idx, sp, n, prep) == -1 :
	    (plan_resolve(idx, n, prep, QPFX_PREFIX, sp->prefix_limit) == -1 ||
	    plan_resolve(idx, n, prep, QPFX_WILD, sp->wildcard_terms) == -1)) {
		return -1;
	}
	for (size_t i = 0; i < n; i++) {
		qprep_t *q = &prep[i];
		bool miss = false;

		if (q->errcode) {
			if (q->n_pfx && !q->compiled) {
				nxs_query_release_scratch(q);	/* (a doc leaf whose doc is not live) */
				q->compiled = true;
			}
			continue;
		}
		if (!q->n_pfx) {
			continue;
		}
		if (nxs_query_splice(q) == -1) {
			nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
			return -1;
		}
		for (size_t j = 0; j < q->n_tokens; j++) {
			miss = miss || !q->tokens[j].term_id;
		}
		if (!miss || !sp->fuzzymatch) {
			(void)nxs_query_compile(q);
			nxs_query_release_scratch(q);
			q->compiled = true;
		}
	}
	return 0;
}

/* parse + lookups (+ compile for the queries without misses) on the worker threads; the misses into *fz.
 * docs != NULL: queries is NULL, query i is the doc leaf of docs[i] (nxs_index_similar) */
int
plan_front(nxs_index_t *idx, const search_params_t *sp, const char *const *queries, const nxs_doc_id_t *docs,
    size_t n, qprep_t *prep, fz_set_t *fz)
{
	nxs_t *nxs = idx->nxs;
	struct nxs_pool *pool = n >= 64 ? nxs_pool_get(nxs) : NULL;
	plan_job_t job = { .idx = idx, .sp = sp, .queries = queries, .docs = docs, .prep = prep, .pc = plan_cache_get(idx) };
	size_t n_fz = 0, fz_len = 0, k = 0, o = 0;

	memset(fz, 0, sizeof(*fz));
	pool_run(pool, plan_parse_chunk, &job, n, 16);
	if ((docs || sp->prefixmatch || sp->wildcardmatch) && plan_prefixes(idx, sp, docs != NULL, n, prep) == -1) {
		return -1;
	}

	for (size_t i = 0; sp->fuzzymatch && i < n; i++) {
		const qprep_t *q = &prep[i];

		for (size_t j = 0; !q->errcode && !q->compiled && !q->cached && j < q->n_tokens; j++) {
			if (!q->tokens[j].term_id) {
				n_fz++;
				fz_len += q->tokens[j].len;
			}
		}
	}
	if (!n_fz) {
		return 0;
	}
	fz->q = malloc(n_fz * sizeof(uint32_t));
	fz->t = malloc(n_fz * sizeof(uint32_t));
	fz->off = malloc((n_fz + 1) * sizeof(uint32_t));
	fz->ids = calloc(n_fz, sizeof(uint32_t));
	fz->bytes = malloc(fz_len + 16);
	if (!fz->q || !fz->t || !fz->off || !fz->ids || !fz->bytes) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		fz_set_free(fz);
		return -1;
	}
	for (size_t i = 0; i < n; i++) {
		qprep_t *q = &prep[i];
		if (q->errcode || q->compiled || q->cached) {
			continue;
		}
		for (size_t j = 0; j < q->n_tokens; j++) {
			const qtok_t *t = &q->tokens[j];
			if (t->term_id) {
				continue;
			}
			fz->q[k] = (uint32_t)i;
			fz->t[k] = (uint32_t)j;
			fz->off[k] = (uint32_t)o;
			memcpy(fz->bytes + o, t->value, t->len);
			o += t->len;
			k++;
		}
	}
	fz->off[k] = (uint32_t)o;
	fz->n = n_fz;
	return 0;
}

/* the winners into the token lists, the remaining queries compiled, the batch's new plans into the cache */
void
plan_back(nxs_index_t *idx, const search_params_t *sp, const char *const *queries,
    size_t n, qprep_t *prep, const fz_set_t *fz)
{
	struct nxs_pool *pool = n >= 64 ? nxs_pool_get(idx->nxs) : NULL;
	struct plan_cache *pc = plan_cache_get(idx);
	plan_job_t job = { .idx = idx, .sp = sp, .queries = queries, .prep = prep, .pc = pc };
	bool second = fz->n != 0;

	for (size_t k = 0; k < fz->n; k++) {
		prep[fz->q[k]].tokens[fz->t[k]].term_id = fz->ids[k];
	}
	for (size_t i = 0; !second && i < n; i++) {
		second = !prep[i].cached && !prep[i].compiled;
	}
	if (second) {
		pool_run(pool, plan_compile_chunk, &job, n, 32);
	}
	/* (this thread only; a query whose string is not at hand -- the late half keeps only the strings it
	 * still has to compile -- was put there by the first half's caller or is not cached) */
	for (size_t i = 0; pc && i < n; i++) {
		const qprep_t *q = &prep[i];
		if (queries && queries[i] && !q->cached && !q->errcode && !q->wide && !q->has_prefix) {
			plan_cache_put(pc, queries[i], strlen(queries[i]), sp->fuzzymatch, q);
		}
	}
}

int
plan_batch(nxs_index_t *idx, const search_params_t *sp, const char *const *queries, const nxs_doc_id_t *docs,
    size_t n, qprep_t *prep)
{
	fz_set_t fz;
	int ret = -1;

	if (plan_front(idx, sp, queries, docs, n, prep, &fz) == -1) {
		return -1;
	}
	if (fz.n) {
		/* one device BK-tree pass for every token that missed */
		(void)late_finish(idx);		/* (a batch whose own pass is still on the device: one pass at a time) */
		if (nxs_index_bk_sync(idx) == -1) {
			goto out;
		}
		if (nxsgpu_fuzzy(idx->dev, fz.bytes, fz.off, (uint32_t)fz.n, fz.ids, NULL) != 0) {
			nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "device fuzzy search failed: %s",
			    nxsgpu_last_error());
			goto out;
		}
	}
	plan_back(idx, sp, queries, n, prep, &fz);
	ret = 0;
out:
	fz_set_free(&fz);
	return ret;
}

void
late_free(struct late_half *lh)
{
	if (lh) {
		fz_set_free(&lh->fz);
		free(lh->qbuf);
		free(lh->queries);
		free(lh);
	}
}

struct late_half *
late_make(const search_params_t *sp, fz_set_t *fz, const char *const *queries, size_t n, const qprep_t *prep)
{
	struct late_half *lh = calloc(1, sizeof(*lh));
	size_t total = 0, o = 0;

	if (!lh) {
		return NULL;
	}
	lh->sp = *sp;
	for (size_t i = 0; i < n; i++) {
		if (!prep[i].cached && !prep[i].compiled && !prep[i].errcode) {
			total += strlen(queries[i]) + 1;
		}
	}
	lh->queries = calloc(n ? n : 1, sizeof(*lh->queries));
	lh->qbuf = malloc(total ? total : 1);
	if (!lh->queries || !lh->qbuf) {
		late_free(lh);
		return NULL;
	}
	for (size_t i = 0; i < n; i++) {
		if (!prep[i].cached && !prep[i].compiled && !prep[i].errcode) {
			const size_t l = strlen(queries[i]) + 1;
			memcpy(lh->qbuf + o, queries[i], l);
			lh->queries[i] = lh->qbuf + o;
			o += l;
		}
	}
	lh->fz = *fz;			/* (moved) */
	memset(fz, 0, sizeof(*fz));
	return lh;
}

int
nxs_index_plan_batch(nxs_index_t *idx, nxs_params_t *params,
    const char *const *queries, size_t n, struct nxsgpu_query *plans_out,
    nxs_err_t *errs)
{
	nxsgpu_query_t *plans = (nxsgpu_query_t *)plans_out;
	search_params_t sp;
	qprep_t *prep;
	int failed = 0;

	nxs_clear_error(idx->nxs);
	if (get_search_params(idx, params, &sp) == -1) {
		return -1;
	}
	if (nxs_index_refresh(idx) == -1) {	/* search.c:309-312 */
		return -1;
	}
	if ((prep = calloc(n ? n : 1, sizeof(qprep_t))) == NULL) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
		return -1;
	}
	if (plan_batch(idx, &sp, queries, NULL, n, prep) == -1) {
		failed = -1;
	}
	for (size_t i = 0; i < n; i++) {
		memset(&plans[i], 0, sizeof(plans[i]));
		if (failed != -1) {
			nxs_err_t code = prep[i].errcode;

			if (!code && prep[i].wide) {
				/* a fixed-size nxsgpu_query_t cannot hold it */
				code = NXS_ERR_LIMIT;
				nxs_decl_err(idx->nxs, code, "query %zu has more than %u terms: "
				    "use nxs_index_search_batch", i, NXSGPU_MAX_TOKENS);
			} else if (code) {
				nxs_decl_err(idx->nxs, code, "%s",
				    prep[i].errmsg ? prep[i].errmsg : "");
			} else if (!prep[i].empty) {
				plans[i] = prep[i].plan;
			}
			failed += code != 0;
			if (errs) {
				errs[i] = code;
			}
		}
		nxs_query_release(&prep[i]);
	}
	free(prep);
	return failed;
}
