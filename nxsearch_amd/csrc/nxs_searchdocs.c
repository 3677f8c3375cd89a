/*
 * nxs_searchdocs.c -- a search within a caller's doc-id set (nxs_index_search_docs, include/nxs.h): the front half
 * of a search as fixed-size plans (plan_batch, as nxs_index_related_batch uses it), every distinct set sorted once
 * on the worker pool (nxs_docset.h), one nxsgpu_search_docs call, and a search's responses from what it returns.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_api_int.h"
#include "nxs_docset.h"

/* a distinct set of the batch: the caller's array, and its sorted copy */
typedef struct {
	const nxs_doc_id_t *src;
	size_t		n;
	uint64_t *	ids;		/* owned: ascending, distinct */
	uint32_t	len;
} docset_t;

/* a query's set as the caller named it, and the plan that uses it */
typedef struct {
	const nxs_doc_id_t *src;
	size_t		n;
	uint32_t	plan;
} setkey_t;

static int
setkey_cmp(const void *a, const void *b)
{
	const setkey_t *x = a, *y = b;

	if (x->src != y->src) {
		return (uintptr_t)x->src < (uintptr_t)y->src ? -1 : 1;
	}
	return x->n < y->n ? -1 : x->n > y->n;
}

static void
docset_sort(void *arg, size_t lo, size_t hi)
{
	docset_t *sets = arg;

	for (size_t s = lo; s < hi; s++) {
		if (sets[s].ids) {
			memcpy(sets[s].ids, sets[s].src, sets[s].n * sizeof(uint64_t));
			sets[s].len = (uint32_t)nxs_ds_sort_unique(sets[s].ids, sets[s].n);
		}
	}
}

int
nxs_index_search_docs_batch(nxs_index_t *idx, nxs_params_t *params, const char *const *queries, size_t n,
    const nxs_doc_id_t *const *docs, const size_t *n_docs, nxs_resp_t **resps, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	nxs_index_t *one[1] = { idx };
	search_params_t sp;
	qprep_t *prep = NULL;
	nxsgpu_query_t *plans = NULL;
	docset_t *sets = NULL;
	setkey_t *keys = NULL;
	const uint64_t **set_ids = NULL;
	uint32_t *slot = NULL, *set_of = NULL, *set_len = NULL, *totals = NULL;
	nxsgpu_results_t res;
	slab_builder_t sb = { 0 };
	size_t np = 0, ns = 0, total = 0;
	bool have_res = false;
	int ret = -1, failed = 0;

	nxs_clear_error(nxs);
	outs_clear(resps, errs, n);
	if (get_search_params(idx, params, &sp) == -1 || lookup_enter(idx, "search_docs", n, false) == -1) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	prep = calloc(n, sizeof(*prep));
	plans = malloc(n * sizeof(*plans));
	sets = calloc(n, sizeof(*sets));
	keys = malloc(n * sizeof(*keys));
	set_ids = calloc(n, sizeof(*set_ids));
	slot = malloc(n * sizeof(*slot));
	set_of = malloc(n * sizeof(*set_of));
	set_len = malloc(n * sizeof(*set_len));
	totals = calloc(n, sizeof(*totals));
	if (!prep || !plans || !sets || !keys || !set_ids || !slot || !set_of || !set_len || !totals) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	if (plan_batch(idx, &sp, queries, NULL, n, prep) == -1) {
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		slot[i] = UINT32_MAX;
		if (!prep[i].errcode && n_docs[i] > NXS_DOCSET_MAX) {
			prep[i].errcode = NXS_ERR_LIMIT;
			prep[i].errmsg = strdup("doc set too large");
		}
		if (!prep[i].errcode && prep[i].wide) {
			char msg[96];

			snprintf(msg, sizeof(msg), "search_docs is not available for a query of more than %u terms", NXSGPU_MAX_TOKENS);
			prep[i].errcode = NXS_ERR_LIMIT;
			prep[i].errmsg = strdup(msg);
		}
		if (prep[i].errcode || prep[i].empty || n_docs[i] == 0 || docs[i] == NULL) {
			continue;
		}
		keys[np].src = docs[i];
		keys[np].n = n_docs[i];
		keys[np].plan = (uint32_t)np;
		slot[i] = (uint32_t)np;
		plans[np++] = prep[i].plan;
	}
	/* queries whose pointer and length are both equal share one set: equal keys are neighbours after a sort */
	qsort(keys, np, sizeof(*keys), setkey_cmp);
	for (size_t k = 0; k < np; k++) {
		if (k == 0 || keys[k].src != keys[k - 1].src || keys[k].n != keys[k - 1].n) {
			sets[ns].src = keys[k].src;
			sets[ns].n = keys[k].n;
			if ((sets[ns].ids = malloc(keys[k].n * sizeof(uint64_t))) == NULL) {
				nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
				goto out;
			}
			ns++;
		}
		set_of[keys[k].plan] = (uint32_t)(ns - 1);
	}
	pool_run(nxs_pool_get(nxs), docset_sort, sets, ns, 1);
	for (size_t s = 0; s < ns; s++) {
		set_ids[s] = sets[s].ids;
		set_len[s] = sets[s].len;
	}
	if (nxsgpu_search_docs(idx->dev, sp.algo, sp.limit, plans, (uint32_t)np, set_ids, set_len, (uint32_t)ns, set_of, &res,
	    totals) != 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "device search_docs pass failed: %s", nxsgpu_last_error());
		goto out;
	}
	have_res = true;
	for (size_t q = 0; q < np; q++) {
		total += res.counts[q];
	}
	if (slab_begin(&sb, n, total) == -1) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		const qprep_t *q = &prep[i];
		nxs_resp_t *rp;

		if (q->errcode) {
			failed++;
			if (errs) {
				errs[i] = q->errcode;
			}
			nxs_decl_err(nxs, q->errcode, "%s", q->errmsg ? q->errmsg : "");
			continue;
		}
		if (slot[i] == UINT32_MAX) {
			rp = slab_resp(&sb, i, 0);	/* resolves to nothing, or an empty set */
		} else {
			const size_t s = slot[i];

			rp = slab_resp(&sb, i, res.counts[s]);
			memcpy(rp->ids, res.doc_ids + res.offsets[s], (size_t)rp->count * sizeof(uint64_t));
			memcpy(rp->scores, res.scores + res.offsets[s], (size_t)rp->count * sizeof(float));
			rp->total = totals[s];
		}
		rp->has_total = sp.total;
		resps[i] = rp;
	}
	/* "explain": the post-hoc pass over the results, as a search's */
	if (sp.explain && sb.slab->refs) {
		ex_item_t *items = malloc(n * sizeof(ex_item_t));
		size_t ni = 0;
		int rc = -1;

		if (!items) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		} else {
			for (size_t i = 0; i < n; i++) {
				if (resps[i]) {
					resps[i]->explained = true;
					if (!prep[i].empty && resps[i]->count) {
						ex_item_of(&items[ni++], resps[i], &prep[i]);
					}
				}
			}
			rc = explain_attach(one, 1, sp.algo, items, ni, sb.slab);
			free(items);
		}
		if (rc != 0) {
			for (size_t i = 0; i < n; i++) {
				resps[i] = NULL;
			}
			slab_free(sb.slab);
			sb.slab = NULL;
			goto out;
		}
	}
	if (sb.slab && sb.slab->refs == 0) {
		slab_free(sb.slab);
	}
	ret = failed;
out:
	if (have_res) {
		nxsgpu_results_free(&res);
	}
	for (size_t i = 0; prep && i < n; i++) {
		nxs_query_release(&prep[i]);
	}
	for (size_t s = 0; sets && s < ns; s++) {
		free(sets[s].ids);
	}
	free(prep);
	free(plans);
	free(sets);
	free(keys);
	free(set_ids);
	free(slot);
	free(set_of);
	free(set_len);
	free(totals);
	return ret;
}

nxs_resp_t *
nxs_index_search_docs(nxs_index_t *idx, nxs_params_t *params, const char *query, size_t len, const nxs_doc_id_t *docs,
    size_t n_docs)
{
	nxs_resp_t *resp = NULL;

	(void)len;	/* (as nxs_index_search: the lexer stops at the NUL byte) */
	(void)nxs_index_search_docs_batch(idx, params, &query, 1, &docs, &n_docs, &resp, NULL);
	return resp;
}
