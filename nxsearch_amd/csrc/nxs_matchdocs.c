/*
 * nxs_matchdocs.c -- a query's matches listed by doc id (nxs_index_match_docs, include/nxs.h): the front half of a
 * search as fixed-size plans (plan_batch, as nxs_index_related_batch and nxs_searchdocs.c use it), one
 * nxsgpu_match_docs call, and the pages as nxs_docs_t objects carved from one slab per batch.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"
#include "nxs_matchdocs.h"

/* one block per batch: this header, the objects [n], the ids of all pages, the query strings; freed with the last
 * object released */
struct docs_slab {
	size_t		refs;
};

struct nxs_docs {
	const nxs_doc_id_t *ids;	/* [count], ascending */
	size_t		count;
	uint64_t	total;		/* |M| */
	bool		more;		/* a doc of M lies beyond the page */
	const char *	query;		/* as given */
	size_t		query_len;
	struct docs_slab *slab;
};

typedef struct {
	struct docs_slab *slab;
	nxs_docs_t *	objs;		/* [n] */
	nxs_doc_id_t *	ids;		/* [total] */
	char *		str;
	size_t		used, str_used;
} docs_builder_t;

static int
docs_begin(docs_builder_t *b, size_t n, size_t total, size_t str_bytes)
{
	const size_t o_objs = (sizeof(struct docs_slab) + 15) & ~(size_t)15;
	const size_t o_ids = (o_objs + n * sizeof(nxs_docs_t) + 15) & ~(size_t)15;
	const size_t o_str = o_ids + total * sizeof(nxs_doc_id_t);
	uint8_t *p = malloc(o_str + str_bytes + 1);

	if (!p) {
		return -1;
	}
	b->slab = (struct docs_slab *)p;
	b->slab->refs = 0;
	b->objs = (nxs_docs_t *)(p + o_objs);
	b->ids = (nxs_doc_id_t *)(p + o_ids);
	b->str = (char *)(p + o_str);
	b->used = b->str_used = 0;
	return 0;
}

/* object i of the slab: `count` ids copied in */
static nxs_docs_t *
docs_make(docs_builder_t *b, size_t i, const char *query, const uint64_t *ids, size_t count, uint64_t total, bool more)
{
	nxs_docs_t *d = &b->objs[i];
	const size_t qlen = strlen(query);

	d->ids = b->ids + b->used;
	if (count) {
		memcpy(b->ids + b->used, ids, count * sizeof(nxs_doc_id_t));
	}
	b->used += count;
	d->count = count;
	d->total = total;
	d->more = more;
	d->query = b->str + b->str_used;
	memcpy(b->str + b->str_used, query, qlen);
	b->str_used += qlen;
	d->query_len = qlen;
	d->slab = b->slab;
	b->slab->refs++;
	return d;
}

size_t
nxs_docs_count(const nxs_docs_t *d)
{
	return d->count;
}

const nxs_doc_id_t *
nxs_docs_ids(const nxs_docs_t *d)
{
	return d->ids;
}

uint64_t
nxs_docs_total(const nxs_docs_t *d)
{
	return d->total;
}

bool
nxs_docs_next(const nxs_docs_t *d, nxs_doc_id_t *from)
{
	if (!d->more || d->count == 0) {
		return false;
	}
	/* (a larger id exists, so this cannot overflow) */
	*from = d->ids[d->count - 1] + 1;
	return true;
}

void
nxs_docs_release(nxs_docs_t *d)
{
	if (d && --d->slab->refs == 0) {
		free(d->slab);
	}
}

/* {"query":"...","docs":[1,5,9],"count":3,"total":120,"next":10} ("next" absent when the set is exhausted) */
char *
nxs_docs_tojson(nxs_docs_t *d, size_t *len)
{
	const size_t cap = 160 + 6 * d->query_len + 21 * d->count;
	nxs_doc_id_t next;
	size_t o = 0;
	char *s;

	if ((s = malloc(cap)) == NULL) {
		return NULL;
	}
	o += (size_t)sprintf(s + o, "{\"query\":");
	o += json_str(s + o, d->query, d->query_len);
	o += (size_t)sprintf(s + o, ",\"docs\":[");
	for (size_t i = 0; i < d->count; i++) {
		o += (size_t)sprintf(s + o, "%s%llu", i ? "," : "", (unsigned long long)d->ids[i]);
	}
	o += (size_t)sprintf(s + o, "],\"count\":%zu,\"total\":%llu", d->count, (unsigned long long)d->total);
	if (nxs_docs_next(d, &next)) {
		o += (size_t)sprintf(s + o, ",\"next\":%llu", (unsigned long long)next);
	}
	s[o++] = '}';
	s[o] = '\0';
	if (len) {
		*len = o;
	}
	return s;
}

/*
 * The front half is a search's (plan_batch: parse, filters, blocking fuzzy / prefix / wildcard resolution, truth
 * table or postfix program).  The fixed-size plans and their cursors go to nxsgpu_match_docs in one call.
 */
int
nxs_index_match_docs_batch(nxs_index_t *idx, nxs_params_t *params, const char *const *queries, size_t n,
    const nxs_doc_id_t *from, nxs_docs_t **out, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	search_params_t sp;
	match_params_t mp;
	qprep_t *prep = NULL;
	nxsgpu_query_t *plans = NULL;
	uint64_t *cursors = NULL, *ids = NULL;
	uint32_t *slot = NULL, *counts = NULL, *totals = NULL;
	uint8_t *more = NULL;
	docs_builder_t db = { 0 };
	size_t np = 0, total = 0, str_bytes = 0, cap;
	int ret = -1, failed = 0;

	nxs_clear_error(nxs);
	outs_clear(out, errs, n);
	if (get_match_params(nxs, params, &mp) == -1 || get_search_params(idx, params, &sp) == -1 ||
	    lookup_enter(idx, "match_docs", n, false) == -1) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	prep = calloc(n, sizeof(*prep));
	plans = malloc(n * sizeof(*plans));
	cursors = malloc(n * sizeof(*cursors));
	slot = malloc(n * sizeof(*slot));
	counts = calloc(n, sizeof(*counts));
	totals = calloc(n, sizeof(*totals));
	more = calloc(n, sizeof(*more));
	if (!prep || !plans || !cursors || !slot || !counts || !totals || !more) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	if (plan_batch(idx, &sp, queries, NULL, n, prep) == -1) {
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		slot[i] = UINT32_MAX;
		if (!prep[i].errcode && !prep[i].wide && !prep[i].empty) {
			slot[i] = (uint32_t)np;
			cursors[np] = from ? from[i] : mp.from;
			plans[np++] = prep[i].plan;
		}
	}
	/* a row of the device call: min(limit, docs of the snapshot) ids (nothing moves between here and the call) */
	cap = nxsgpu_index_docs(idx->dev) < mp.limit ? (size_t)nxsgpu_index_docs(idx->dev) : mp.limit;
	if (np) {
		if ((ids = malloc((np * cap + 1) * sizeof(*ids))) == NULL) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
			goto out;
		}
		if (nxsgpu_match_docs(idx->dev, sp.algo, plans, (uint32_t)np, cursors, mp.limit, ids, counts, more, totals) != 0) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "device match_docs pass failed: %s", nxsgpu_last_error());
			goto out;
		}
	}
	for (size_t i = 0; i < n; i++) {
		if (slot[i] != UINT32_MAX) {
			total += counts[slot[i]];
		}
		str_bytes += strlen(queries[i]);
	}
	if (docs_begin(&db, n, total, str_bytes) == -1) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		nxs_err_t code = prep[i].errcode;
		const size_t s = slot[i];

		if (code) {
			/* what a search reports for the string */
			nxs_decl_err(nxs, code, "%s", prep[i].errmsg ? prep[i].errmsg : "");
		} else if (prep[i].wide) {
			code = NXS_ERR_LIMIT;
			nxs_decl_err(nxs, code, "match_docs is not available for a query of more than %u terms", NXSGPU_MAX_TOKENS);
		} else if (s == UINT32_MAX) {
			/* resolves to nothing: an empty page */
			out[i] = docs_make(&db, i, queries[i], NULL, 0, 0, false);
		} else {
			out[i] = docs_make(&db, i, queries[i], ids + s * cap, counts[s], totals[s], more[s] != 0);
		}
		if (!out[i]) {
			if (errs) {
				errs[i] = code;
			}
			failed++;
		}
	}
	if (db.slab->refs == 0) {
		free(db.slab);
	}
	ret = failed;
out:
	for (size_t i = 0; prep && i < n; i++) {
		nxs_query_release(&prep[i]);
	}
	free(prep);
	free(plans);
	free(cursors);
	free(ids);
	free(slot);
	free(counts);
	free(totals);
	free(more);
	return ret;
}

nxs_docs_t *
nxs_index_match_docs(nxs_index_t *idx, nxs_params_t *params, const char *query, size_t len)
{
	nxs_docs_t *d = NULL;

	(void)len;	/* (as nxs_index_search: the lexer stops at the NUL byte) */
	(void)nxs_index_match_docs_batch(idx, params, &query, 1, NULL, &d, NULL);
	return d;
}

#ifdef NXS_TEST_HOOKS
/* the parameters as nxs_index_match_docs reads its own keys: 0, or -1 with the error declared */
int
nxs_test_match_params(nxs_t *nxs, nxs_params_t *params, unsigned *limit, uint64_t *from)
{
	match_params_t mp;

	nxs_clear_error(nxs);
	if (get_match_params(nxs, params, &mp) == -1) {
		return -1;
	}
	*limit = mp.limit;
	*from = mp.from;
	return 0;
}

/* an nxs_docs_t built by hand (a slab of one) */
nxs_docs_t *
nxs_test_docs_build(const char *query, const uint64_t *ids, size_t count, uint64_t total, bool more)
{
	docs_builder_t db = { 0 };

	if (docs_begin(&db, 1, count, strlen(query)) == -1) {
		return NULL;
	}
	return docs_make(&db, 0, query, ids, count, total, more);
}
#endif /* NXS_TEST_HOOKS */
