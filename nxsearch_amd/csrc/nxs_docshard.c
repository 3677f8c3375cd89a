/*
 * nxs_docshard.c -- doc-sharded collections (N4): the search over the shards of
 * a collection, in one process or one rank per shard, and following the files
 * (nxs_docshard_refresh[_rank]).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"

/* collection-wide df = sum of the shards' (in a multi-process deployment: an
 * all-reduce of the same arrays); every shard then recomputes its impacts */
static int
docshard_set_global_df(nxs_index_t *const *shards, unsigned n_shards)
{
	nxs_t *nxs = shards[0]->nxs;
	const uint32_t T = shards[0]->last_id;
	uint32_t *sum = calloc((size_t)T + 2, sizeof(uint32_t));
	uint32_t *df = calloc((size_t)T + 2, sizeof(uint32_t));
	int ret = -1;

	if (!sum || !df) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	for (unsigned s = 0; s < n_shards; s++) {
		if (shards[s]->last_id != T || shards[s]->n_shards != n_shards || shards[s]->shard != s) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "the indexes are not shards 0..%u of one collection",
			    n_shards - 1);
			goto out;
		}
		(void)nxsgpu_index_df(shards[s]->dev, df);
		for (uint32_t t = 1; t <= T; t++) {
			sum[t] += df[t];
		}
	}
	for (unsigned s = 0; s < n_shards; s++) {
		if (nxsgpu_index_set_global_df(shards[s]->dev, sum, T) != 0) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "%s", nxsgpu_last_error());
			goto out;
		}
		shards[s]->global_df_set = true;
	}
	ret = 0;
out:
	free(sum);
	free(df);
	return ret;
}

/*
 * One shard's pass: the candidates its heap accepts for every plan of the batch
 * (nxsgpu_search_candidates), on the shard's own device and streams.  Shards of
 * one process run these side by side, one host thread each (the HIP side keeps
 * its error text per thread).
 */
typedef struct {
	nxs_index_t *	shard;
	int		algo;
	uint64_t	limit;
	const nxsgpu_query_t *plans;
	uint32_t	np, cap;
	uint64_t *	ids;	/* [np][cap] */
	float *		sc;
	uint32_t *	cnt;	/* [np] */
	uint32_t *	tot;	/* [np] the shard's total match counts, or NULL */
	int		ret;
	char		err[256];
} ds_job_t;

static void *
ds_job_run(void *arg)
{
	ds_job_t *j = arg;

	j->ret = nxsgpu_search_candidates(j->shard->dev, j->algo, j->limit, j->plans, j->np, j->cap,
	    j->ids, j->sc, j->cnt);
	if (j->ret == 0 && j->tot) {
		j->ret = nxsgpu_count(j->shard->dev, j->algo, j->plans, j->np, j->tot);
	}
	if (j->ret != 0) {
		snprintf(j->err, sizeof(j->err), "%s", nxsgpu_last_error());
	}
	return NULL;
}

/*
 * The doc-sharded search (N4).  Two forms share everything but where the other
 * shards' candidates come from:
 *  - in-process (nxs_docshard_search_batch): `local` holds ALL n_shards shard
 *    indexes, each on its own device / streams; their passes run concurrently
 *    (one host thread per shard), then the merge;
 *  - one process per shard (nxs_docshard_search_batch_rank): `local` is this
 *    rank's shard; the ranks all-gather their candidate blocks
 *    (u32 abort | u32 cnt[np] | u64 ids[np][cap] | f32 sc[np][cap]) through the
 *    communicator attached with nxs_index_shard() and EVERY rank merges -- the
 *    query-sharded mode's rule: one collective per step, all ranks hold all
 *    responses.  `gathered` (tests): the blocks of all ranks, instead of a
 *    communicator; `my_block` (tests): hand out this rank's block and stop.
 * The merge feeds the shards' accepted-candidate logs, highest doc ids first,
 * through the reference's heap once more (nxsgpu_merge_candidates).
 */
static size_t
ds_block_bytes(size_t np, uint32_t cap)
{
	return 8 + ((np * 4 + 7) & ~(size_t)7) + np * cap * 8 + np * cap * 4;
}

static int
docshard_search(nxs_index_t *const *local, unsigned n_local, unsigned n_shards, unsigned my_shard,
    nxs_params_t *params, const char *const *queries, size_t n, nxs_resp_t **resps, nxs_err_t *errs,
    uint32_t cap0, const uint8_t *gathered, uint8_t **my_block, size_t *my_block_len, bool rank_form)
{
	nxs_index_t *idx0 = local[0];
	nxs_t *nxs = idx0->nxs;
	const bool ranks = n_local == 1 && n_shards > 1;	/* one process per shard */
	search_params_t sp;
	qprep_t *prep = NULL;
	nxsgpu_query_t *plans = NULL;
	uint32_t *plan_of = NULL, *cnt_all = NULL, *o_cnt = NULL;
	uint64_t *ids_all = NULL, *o_ids = NULL;
	float *sc_all = NULL, *o_sc = NULL;
	ds_job_t *jobs = NULL;
	pthread_t *thr = NULL;
	uint8_t *sendb = NULL, *recvb = NULL;
	slab_builder_t sb = { 0 };
	size_t np = 0, total = 0;
	uint32_t cap = cap0 ? cap0 : 512;
	int failed = 0, ret = -1;

	nxs_clear_error(nxs);
	outs_clear(resps, errs, n);
	if (get_search_params(idx0, params, &sp) == -1) {
		return -1;
	}
	if (sp.limit > NXSGPU_BIG_K) {
		nxs_decl_err(nxs, NXS_ERR_LIMIT, "doc-sharded search takes limit <= %d", NXSGPU_BIG_K);
		return -1;
	}
	/* (the rank form: the totals would have to travel in the candidate blocks; include/nxs.h) */
	if (sp.total && (rank_form || ranks || gathered || my_block)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "total is not available on a sharded batch");
		return -1;
	}
	/* (the rank form: a rank holds one shard, so the rows of the other shards' docs would have to travel in a
	 * collective of their own; every rank passes the same params, so every rank refuses) */
	if (sp.explain && (rank_form || ranks || gathered || my_block)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "explain is not available on a ranked doc-shard batch");
		return -1;
	}
	for (unsigned s = 0; s < n_local; s++) {
		/* (rank form: every rank carries the mark, so none enters the collective) */
		if (local[s]->ds_inconsistent) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "the doc-sharded collection is inconsistent after a failed "
			    "refresh: refresh it (nxs_docshard_refresh)");
			return -1;
		}
	}
	/* a shard's heap accepts ~ k (1 + ln(matches / k)) items: room for that from the start (a log that
	 * overflows costs a second pass over every shard) */
	if (!cap0 && sp.limit > NXSGPU_FAST_K) {
		cap = (uint32_t)(sp.limit * 8 < 32768 ? sp.limit * 8 : 32768);
	}
	if (!idx0->global_df_set) {
		if (!ranks && docshard_set_global_df(local, n_shards) == -1) {
			return -1;
		}
		if (ranks) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "nxs_docshard_attach() the shard first (collection-wide df)");
			return -1;
		}
	}
	if (n == 0) {
		return 0;
	}
	prep = calloc(n, sizeof(qprep_t));
	plans = calloc(n, sizeof(nxsgpu_query_t));
	plan_of = calloc(n, sizeof(uint32_t));
	jobs = calloc(n_local, sizeof(ds_job_t));
	thr = calloc(n_local, sizeof(pthread_t));
	if (!prep || !plans || !plan_of || !jobs || !thr) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	/* the term dictionary and the BK-tree are the same on every shard */
	if (plan_batch(idx0, &sp, queries, NULL, n, prep) == -1) {
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		if (!prep[i].errcode && prep[i].wide) {
			prep[i].errcode = NXS_ERR_LIMIT;
			prep[i].errmsg = strdup("doc-sharded search takes at most 32 query terms");
		}
		if (!prep[i].errcode && !prep[i].empty) {
			plan_of[i] = (uint32_t)np;
			plans[np++] = prep[i].plan;
		}
	}
	o_ids = malloc((np ? np : 1) * sp.limit * sizeof(uint64_t));
	o_sc = malloc((np ? np : 1) * sp.limit * sizeof(float));
	o_cnt = calloc(np ? np : 1, sizeof(uint32_t));
	for (;;) {
		bool overflow = false;
		const size_t per = (np ? np : 1) * (size_t)cap;
		const size_t bb = ds_block_bytes(np, cap);

		free(ids_all); free(sc_all); free(cnt_all);
		ids_all = malloc(per * n_shards * sizeof(uint64_t));
		sc_all = malloc(per * n_shards * sizeof(float));
		cnt_all = calloc((np ? np : 1) * (size_t)n_shards, sizeof(uint32_t));
		for (unsigned s = 0; s < n_local; s++) {
			free(jobs[s].ids); free(jobs[s].sc); free(jobs[s].cnt);
			jobs[s].ids = malloc(per * sizeof(uint64_t));
			jobs[s].sc = malloc(per * sizeof(float));
			jobs[s].cnt = calloc(np ? np : 1, sizeof(uint32_t));
			if (sp.total && !jobs[s].tot) {
				jobs[s].tot = calloc(np ? np : 1, sizeof(uint32_t));
			}
			if (!jobs[s].ids || !jobs[s].sc || !jobs[s].cnt || (sp.total && !jobs[s].tot)) {
				o_cnt = (free(o_cnt), NULL);
			}
			jobs[s].shard = local[s];
			jobs[s].algo = sp.algo;
			jobs[s].limit = sp.limit;
			jobs[s].plans = plans;
			jobs[s].np = (uint32_t)np;
			jobs[s].cap = cap;
			jobs[s].ret = 0;
		}
		if (!o_ids || !o_sc || !o_cnt || !ids_all || !sc_all || !cnt_all) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
			goto out;
		}
		/* every local shard's pass is queued before any is waited for */
		if (np) {
			unsigned started = 0;
			for (unsigned s = 1; s < n_local; s++) {
				if (pthread_create(&thr[s], NULL, ds_job_run, &jobs[s]) != 0) {
					break;
				}
				started = s;
			}
			ds_job_run(&jobs[0]);
			for (unsigned s = 1; s <= started; s++) {
				(void)pthread_join(thr[s], NULL);
			}
			for (unsigned s = started + 1; s < n_local; s++) {
				ds_job_run(&jobs[s]);	/* (no thread: in line) */
			}
		}
		for (unsigned s = 0; s < n_local; s++) {
			if (jobs[s].ret != 0) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "device search failed: %s", jobs[s].err);
				if (!ranks) {
					goto out;
				}
			}
		}
		if (!ranks) {
			/* [query][shard][cap]: what the merge works on */
			for (unsigned s = 0; s < n_local; s++) {
				for (size_t q = 0; q < np; q++) {
					const size_t at = (q * n_shards + s) * cap;
					overflow = overflow || jobs[s].cnt[q] > cap;
					cnt_all[q * n_shards + s] = jobs[s].cnt[q];
					memcpy(ids_all + at, jobs[s].ids + q * cap, (size_t)cap * sizeof(uint64_t));
					memcpy(sc_all + at, jobs[s].sc + q * cap, (size_t)cap * sizeof(float));
				}
			}
		} else {
			/* this rank's block; a rank whose pass failed says so in the first word
			 * and still takes part in the collective */
			free(sendb); free(recvb);
			sendb = calloc(1, bb);
			recvb = malloc(bb * n_shards);
			if (!sendb || !recvb) {
				nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
				goto out;
			}
			const size_t cnt_len = (np * 4 + 7) & ~(size_t)7;
			((uint32_t *)sendb)[0] = jobs[0].ret != 0 ? (uint32_t)NXS_ERR_FATAL : 0u;
			memcpy(sendb + 8, jobs[0].cnt, np * 4);
			memcpy(sendb + 8 + cnt_len, jobs[0].ids, np * (size_t)cap * 8);
			memcpy(sendb + 8 + cnt_len + np * (size_t)cap * 8, jobs[0].sc, np * (size_t)cap * 4);
			if (my_block) {			/* tests: one rank at a time, no collective */
				*my_block = sendb;
				*my_block_len = bb;
				sendb = NULL;
				ret = 0;
				goto out;
			}
			if (gathered) {
				memcpy(recvb, gathered, bb * n_shards);
			} else if (nxsgpu_comm_allgather(idx0->comm, sendb, recvb, bb) != 0) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "all-gather failed: %s", nxsgpu_last_error());
				goto out;
			}
			for (unsigned s = 0; s < n_shards; s++) {
				const uint8_t *blk = recvb + (size_t)s * bb;
				const uint32_t *bc = (const uint32_t *)(blk + 8);

				if (((const uint32_t *)blk)[0]) {
					if (s != my_shard || !nxs->errcode) {
						nxs_decl_err(nxs, NXS_ERR_FATAL, "shard %u failed its pass of the batch", s);
					}
					goto out;	/* every rank sees it: all fail together */
				}
				for (size_t q = 0; q < np; q++) {
					const size_t at = (q * n_shards + s) * cap;
					overflow = overflow || bc[q] > cap;
					cnt_all[q * n_shards + s] = bc[q];
					memcpy(ids_all + at, blk + 8 + cnt_len + q * (size_t)cap * 8, (size_t)cap * 8);
					memcpy(sc_all + at, blk + 8 + cnt_len + np * (size_t)cap * 8 + q * (size_t)cap * 4, (size_t)cap * 4);
				}
			}
		}
		if (!overflow) {
			break;
		}
		if (cap >= (1u << 16) || gathered || my_block) {
			nxs_decl_err(nxs, NXS_ERR_LIMIT, "candidate log overflow");
			goto out;
		}
		cap *= 8;	/* rare: adversarial score orders; try again with room (every rank
				 * sees every count: all ranks retry together) */
	}
	if (np && nxsgpu_merge_candidates(idx0->device, (uint32_t)sp.limit, (uint32_t)np, n_shards, cap,
	    ids_all, sc_all, cnt_all, o_ids, o_sc, o_cnt) != 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "merge failed: %s", nxsgpu_last_error());
		goto out;
	}
	for (size_t q = 0; q < np; q++) {
		total += o_cnt[q];
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
		if (q->empty) {
			resps[i] = slab_resp(&sb, i, 0);
			continue;
		}
		rp = slab_resp(&sb, i, o_cnt[plan_of[i]]);
		memcpy(rp->ids, o_ids + (size_t)plan_of[i] * sp.limit, (size_t)rp->count * sizeof(uint64_t));
		memcpy(rp->scores, o_sc + (size_t)plan_of[i] * sp.limit, (size_t)rp->count * sizeof(float));
		resps[i] = rp;
	}
	/* the shards hold disjoint docs: a query's total is the sum of the shards' */
	for (size_t i = 0; sp.total && i < n; i++) {
		if (resps[i]) {
			resps[i]->has_total = true;
			for (unsigned s = 0; !prep[i].empty && s < n_local; s++) {
				resps[i]->total += jobs[s].tot[plan_of[i]];
			}
		}
	}
	/* "explain": every shard is asked about the merged results; a row comes from the shard that holds the doc */
	if (sp.explain && sb.slab->refs) {
		ex_item_t *items = malloc(n * sizeof(ex_item_t));
		size_t ni = 0;
		int rc;

		if (!items) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
			rc = -1;
		} else {
			for (size_t i = 0; i < n; i++) {
				if (resps[i]) {
					resps[i]->explained = true;
					if (!prep[i].empty && resps[i]->count) {
						ex_item_of(&items[ni++], resps[i], &prep[i]);
					}
				}
			}
			rc = explain_attach(local, n_local, sp.algo, items, ni, sb.slab);
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
	for (size_t i = 0; prep && i < n; i++) {
		nxs_query_release(&prep[i]);
	}
	for (unsigned s = 0; jobs && s < n_local; s++) {
		free(jobs[s].ids); free(jobs[s].sc); free(jobs[s].cnt); free(jobs[s].tot);
	}
	free(jobs); free(thr); free(sendb); free(recvb);
	free(prep); free(plans); free(plan_of);
	free(ids_all); free(sc_all); free(cnt_all);
	free(o_ids); free(o_sc); free(o_cnt);
	return ret;
}

int
nxs_docshard_search_batch(nxs_index_t *const *shards, unsigned n_shards, nxs_params_t *params,
    const char *const *queries, size_t n, nxs_resp_t **resps, nxs_err_t *errs)
{
	return docshard_search(shards, n_shards, n_shards, 0, params, queries, n, resps, errs, 0, NULL, NULL, NULL, false);
}

/*
 * One process per shard: make this rank's shard part of the collection.  The
 * communicator is the one nxs_index_shard() attached (rank r holds shard r of
 * `world`); collection-wide df = the all-gathered shards' df arrays, summed, and
 * every impact of the shard is recomputed with it.  Collective.
 */
int
nxs_docshard_attach(nxs_index_t *shard)
{
	nxs_t *nxs = shard->nxs;
	const uint32_t T = shard->last_id;
	const unsigned W = shard->n_shards;
	uint32_t *df = NULL, *all = NULL;
	int ret = -1;

	nxs_clear_error(nxs);
	if (W > 1 && (!shard->comm || nxsgpu_comm_world(shard->comm) != (int)W ||
	    nxsgpu_comm_rank(shard->comm) != (int)shard->shard)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "shard %u of %u needs a communicator of %u ranks with itself as "
		    "rank %u (nxs_index_shard)", shard->shard, W, W, shard->shard);
		return -1;
	}
	df = calloc((size_t)T + 2, sizeof(uint32_t));
	all = calloc(((size_t)T + 2) * W, sizeof(uint32_t));
	if (!df || !all) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	(void)nxsgpu_index_df(shard->dev, df);
	if (W > 1) {
		if (nxsgpu_comm_allgather(shard->comm, df, all, ((size_t)T + 2) * 4) != 0) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "all-gather of the shards' df failed: %s", nxsgpu_last_error());
			goto out;
		}
		memset(df, 0, ((size_t)T + 2) * 4);
		for (unsigned r = 0; r < W; r++) {
			for (uint32_t t = 1; t <= T; t++) {
				df[t] += all[(size_t)r * (T + 2) + t];
			}
		}
	}
	if (nxsgpu_index_set_global_df(shard->dev, df, T) != 0) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "%s", nxsgpu_last_error());
		goto out;
	}
	shard->global_df_set = true;
	ret = 0;
out:
	free(df);
	free(all);
	return ret;
}

int
nxs_docshard_search_batch_rank(nxs_index_t *shard, nxs_params_t *params,
    const char *const *queries, size_t n, nxs_resp_t **resps, nxs_err_t *errs)
{
	nxs_index_t *local[1] = { shard };

	if (shard->n_shards > 1 && !shard->comm) {
		nxs_clear_error(shard->nxs);
		nxs_decl_err(shard->nxs, NXS_ERR_INVALID, "no communicator attached (nxs_index_shard)");
		return -1;
	}
	return docshard_search(local, 1, shard->n_shards, shard->shard, params, queries, n, resps, errs, 0, NULL, NULL, NULL, true);
}

/* ---- N4: following the files (nxs_docshard_refresh[_rank]) ------------------------ */

/*
 * The record every rank contributes to a refresh (u64 words): its snapshot of the
 * files, the highest doc id it holds, whether it could take part at all and
 * whether it carries the "inconsistent" mark of a failed refresh.
 */
enum { DSR_TERMS, DSR_DTMAP, DSR_DOCS, DSR_TOKENS, DSR_MAXID, DSR_STATUS, DSR_REBUILD, DSR_WORDS = 8 };

static void
dsr_record(nxs_index_t *idx, uint64_t rec[DSR_WORDS])
{
	nxs_snap_t sn;

	memset(rec, 0, DSR_WORDS * sizeof(uint64_t));
	if (!idx->tmap || !idx->dmap || !idx->dev) {
		rec[DSR_STATUS] = NXS_ERR_FATAL;
		return;
	}
	nxs_index_snapshot(idx, &sn);
	rec[DSR_TERMS] = sn.terms_len;
	rec[DSR_DTMAP] = sn.dtmap_len;
	rec[DSR_DOCS] = sn.hdr_docs;
	rec[DSR_TOKENS] = sn.hdr_tokens;
	rec[DSR_MAXID] = idx->n_ord ? idx->h_doc_ids[idx->n_ord - 1] : 0;
	rec[DSR_REBUILD] = idx->ds_inconsistent;
}

static const uint64_t *
dsr_consumed(const nxs_index_t *idx, uint64_t c[4])
{
	c[0] = idx->terms_consumed;
	c[1] = idx->dt_consumed;
	c[2] = idx->hdr_docs_seen;
	c[3] = idx->hdr_tokens_seen;
	return c;
}

/*
 * Rank protocol, step 1, on the gathered records (a pure function: every rank
 * computes the same answer).  The snapshot is the record with the largest
 * nxsdtmap length, the lowest rank on ties -- the ranks share the files, so by
 * now every rank's view reaches at least that far; the collection's highest doc
 * id is the largest any rank holds.  -1: a rank could not take part; 0: no
 * record differs from what was consumed (`consumed`: terms, dtmap, docs, tokens)
 * and no rank is marked inconsistent; 1: refresh to `out`
 * (out[DSR_REBUILD]: a full rebuild is due).
 */
static int
dsr_agree(const uint64_t *recs, unsigned W, const uint64_t consumed[4], uint64_t out[DSR_WORDS])
{
	unsigned best = 0;
	uint64_t max_id = 0;
	bool moved = false, rebuild = false;

	for (unsigned r = 0; r < W; r++) {
		const uint64_t *x = recs + (size_t)r * DSR_WORDS;

		if (x[DSR_STATUS]) {
			return -1;
		}
		if (x[DSR_DTMAP] > recs[(size_t)best * DSR_WORDS + DSR_DTMAP]) {
			best = r;
		}
		for (unsigned w = 0; w < 4; w++) {
			moved = moved || x[w] != consumed[w];
		}
		rebuild = rebuild || x[DSR_REBUILD];
		max_id = x[DSR_MAXID] > max_id ? x[DSR_MAXID] : max_id;
	}
	memcpy(out, recs + (size_t)best * DSR_WORDS, DSR_WORDS * sizeof(uint64_t));
	out[DSR_MAXID] = max_id;
	out[DSR_REBUILD] = rebuild;
	return moved || rebuild ? 1 : 0;
}

static void
dsr_snap(const uint64_t agreed[DSR_WORDS], nxs_snap_t *sn)
{
	sn->terms_len = agreed[DSR_TERMS];
	sn->dtmap_len = agreed[DSR_DTMAP];
	sn->hdr_docs = agreed[DSR_DOCS];
	sn->hdr_tokens = agreed[DSR_TOKENS];
}

/* a shard's host walk to the agreed snapshot: 0 delta in *rd, 1 rebuild, -1 error */
static int
dsr_walk(nxs_index_t *idx, const uint64_t agreed[DSR_WORDS], nxs_delta_t **rd)
{
	nxs_snap_t sn;

	dsr_snap(agreed, &sn);
	/* appended docs (ids above every loaded one) go to the last shard */
	return nxs_shard_walk(idx, &sn, agreed[DSR_MAXID], idx->shard + 1 >= idx->n_shards, rd);
}

/* a shard's device step: merge its delta (impacts deferred), or with rd == NULL
 * rebuild its slice of the agreed snapshot; 0 / -1 */
static int
dsr_device_step(nxs_index_t *idx, const uint64_t agreed[DSR_WORDS], nxs_delta_t *rd)
{
	nxs_snap_t sn;

	if (idx->test_fail_dsref && --idx->test_fail_dsref == 0) {
		nxs_delta_abort(idx, rd);
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "shard %u: injected failure of the refresh's device step", idx->shard);
		return -1;
	}
	if (rd) {
		return nxs_shard_merge(idx, rd);
	}
	dsr_snap(agreed, &sn);
	return nxs_shard_rebuild(idx, &sn);
}

/*
 * In-process form: all shards of the collection.  One snapshot (four loads,
 * shard 0's mapping); every shard walks and validates on the host before any
 * device state changes; then every shard merges (or, if any shard needs it,
 * every shard rebuilds its slice); then the collection-wide df is summed and
 * every shard's impacts are recomputed once.  A failure after the first device
 * step marks the collection inconsistent.
 */
int
nxs_docshard_refresh(nxs_index_t *const *shards, unsigned n_shards)
{
	nxs_t *nxs;
	uint64_t *recs = NULL, agreed[DSR_WORDS], consumed[4];
	nxs_delta_t **deltas = NULL;
	bool rebuild;
	int r, ret = -1;

	if (!shards || n_shards == 0 || !shards[0]) {
		return -1;
	}
	nxs = shards[0]->nxs;
	nxs_clear_error(nxs);
	for (unsigned s = 0; s < n_shards; s++) {
		if (!shards[s] || shards[s]->n_shards != n_shards || shards[s]->shard != s) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "the indexes are not shards 0..%u of one collection", n_shards - 1);
			return -1;
		}
		if (pend_oldest(shards[s])) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "batches are in flight");
			return -1;
		}
	}
	recs = calloc((size_t)n_shards * DSR_WORDS, sizeof(uint64_t));
	deltas = calloc(n_shards, sizeof(*deltas));
	if (!recs || !deltas) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	dsr_record(shards[0], recs);		/* the snapshot: read once */
	for (unsigned s = 1; s < n_shards; s++) {
		uint64_t *x = recs + (size_t)s * DSR_WORDS;
		memcpy(x, recs, DSR_MAXID * sizeof(uint64_t));
		x[DSR_MAXID] = shards[s]->n_ord ? shards[s]->h_doc_ids[shards[s]->n_ord - 1] : 0;
		x[DSR_STATUS] = recs[DSR_STATUS];
		x[DSR_REBUILD] = shards[s]->ds_inconsistent;
	}
	if ((r = dsr_agree(recs, n_shards, dsr_consumed(shards[0], consumed), agreed)) <= 0) {
		if (r < 0) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "a shard holds no snapshot");
		}
		ret = r;
		goto out;
	}
	rebuild = agreed[DSR_REBUILD] != 0;
	for (unsigned s = 0; s < n_shards && !rebuild; s++) {
		if ((r = dsr_walk(shards[s], agreed, &deltas[s])) < 0) {
			goto fail;	/* (the dictionaries of the shards before it moved on) */
		}
		rebuild = r == 1;
	}
	for (unsigned s = 0; s < n_shards; s++) {
		nxs_delta_t *rd = rebuild ? NULL : deltas[s];

		if (rebuild) {
			nxs_delta_abort(shards[s], deltas[s]);
		}
		deltas[s] = NULL;
		if (dsr_device_step(shards[s], agreed, rd) != 0) {
			goto fail;
		}
	}
	for (unsigned s = 1; s < n_shards; s++) {
		if (shards[s]->dt_consumed != shards[0]->dt_consumed) {
			/* a rebuild stopped at different blocks (one names a term nxsterms does not hold yet) */
			nxs_decl_err(nxs, NXS_ERR_FATAL, "the shards consumed different parts of the dtmap index");
			goto fail;
		}
	}
	if (docshard_set_global_df(shards, n_shards) != 0) {
		goto fail;
	}
	for (unsigned s = 0; s < n_shards; s++) {
		shards[s]->ds_inconsistent = false;
	}
	ret = 1;
	goto out;
fail:
	for (unsigned s = 0; s < n_shards; s++) {
		nxs_delta_abort(shards[s], deltas[s]);
		deltas[s] = NULL;
		shards[s]->ds_inconsistent = true;
	}
	if (nxs->errcode == NXS_ERR_SUCCESS) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "doc-shard refresh failed");
	}
out:
	free(recs);
	free(deltas);
	return ret;
}

/*
 * Rank form, the phases between the collectives (the test hooks play them one
 * rank after another).  The block a rank hands to the df all-gather:
 * u32 status | u32 mode (1 merged, 2 rebuilt) | u32 T | u32 0 | u64 dtmap consumed |
 * u64 0 | u32 df[cap], cap = agreed nxsterms length / 16 + 2 (a term block takes at
 * least 16 bytes: every rank's T fits, and every rank knows the size).
 */
#define	DSB_HDR	32

static size_t
dsb_bytes(const uint64_t agreed[DSR_WORDS])
{
	return DSB_HDR + (agreed[DSR_TERMS] / 16 + 2) * 4;
}

/* step 1 -> step 3: agree, walk, device merge (impacts deferred), this rank's block.
 * -1: a rank could not take part (every rank returns -1); 0: nothing moved; 1: *blk */
static int
dsr_merge_phase(nxs_index_t *idx, const uint64_t *recs, unsigned W, uint8_t **blk, size_t *len)
{
	uint64_t agreed[DSR_WORDS], consumed[4];
	nxs_delta_t *rd = NULL;
	uint32_t *h;
	int r, mode;

	*blk = NULL;
	*len = 0;
	if ((r = dsr_agree(recs, W, dsr_consumed(idx, consumed), agreed)) <= 0) {
		if (r < 0) {
			nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "a shard could not take part in the refresh");
		}
		return r;
	}
	*len = dsb_bytes(agreed);
	if ((*blk = calloc(1, *len)) == NULL) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
		return -1;
	}
	h = (uint32_t *)*blk;
	mode = agreed[DSR_REBUILD] ? 2 : 1;
	if (mode == 1 && (r = dsr_walk(idx, agreed, &rd)) != 0) {
		mode = r == 1 ? 2 : 0;
	}
	if (mode == 0 || dsr_device_step(idx, agreed, mode == 1 ? rd : NULL) != 0) {
		h[0] = NXS_ERR_FATAL;		/* still takes part: every rank learns of it */
		return 1;
	}
	if ((size_t)idx->last_id + 2 > (*len - DSB_HDR) / 4) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "shard %u: %u terms beyond the snapshot", idx->shard, idx->last_id);
		h[0] = NXS_ERR_FATAL;
		return 1;
	}
	h[1] = (uint32_t)mode;
	h[2] = idx->last_id;
	memcpy(*blk + 16, &idx->dt_consumed, 8);
	(void)nxsgpu_index_df(idx->dev, (uint32_t *)(*blk + DSB_HDR));
	return 1;
}

/* step 3 -> 4: every rank's block; the summed df, one impact pass.  0, or the failure
 * this rank reports to the final exchange */
static uint32_t
dsr_finish(nxs_index_t *idx, const uint8_t *all, unsigned W, size_t len)
{
	const uint32_t *h0 = (const uint32_t *)all;
	const uint32_t T = h0[2];
	uint32_t *sum;

	for (unsigned r = 0; r < W; r++) {
		const uint8_t *b = all + (size_t)r * len;
		const uint32_t *h = (const uint32_t *)b;

		if (h[0] || h[1] != h0[1] || h[2] != T || memcmp(b + 16, all + 16, 8) != 0) {
			if (idx->nxs->errcode == NXS_ERR_SUCCESS) {
				nxs_decl_err(idx->nxs, NXS_ERR_FATAL, h[0] ? "shard %u failed its part of the refresh" :
				    "shard %u reached a different state in the refresh", r);
			}
			return NXS_ERR_FATAL;
		}
	}
	if (T != idx->last_id || (sum = calloc((size_t)T + 2, sizeof(uint32_t))) == NULL) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "shard %u: the collection-wide df does not fit", idx->shard);
		return NXS_ERR_FATAL;
	}
	for (unsigned r = 0; r < W; r++) {
		const uint32_t *df = (const uint32_t *)(all + (size_t)r * len + DSB_HDR);
		for (uint32_t t = 1; t <= T; t++) {
			sum[t] += df[t];
		}
	}
	if (nxsgpu_index_set_global_df(idx->dev, sum, T) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "shard %u: %s", idx->shard, nxsgpu_last_error());
		free(sum);
		return NXS_ERR_FATAL;
	}
	free(sum);
	idx->global_df_set = true;
	return 0;
}

/* after the final exchange of the ranks' finish status: 1 all done, -1 marked inconsistent */
static int
dsr_settle(nxs_index_t *idx, const uint32_t *fin, unsigned W)
{
	for (unsigned r = 0; r < W; r++) {
		if (fin[r]) {
			idx->ds_inconsistent = true;
			if (idx->nxs->errcode == NXS_ERR_SUCCESS) {
				nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "shard %u failed the refresh: the collection is "
				    "inconsistent until the next refresh", r);
			}
			return -1;
		}
	}
	idx->ds_inconsistent = false;
	return 1;
}

/*
 * One process per shard (collective over the communicator of nxs_index_shard):
 * all-gather of the snapshot records (the only collective when nothing moved),
 * agree + walk + merge, all-gather of the df blocks (with each rank's status),
 * one impact pass with the summed df, all-gather of the outcome.  Every rank
 * returns the same value.
 */
static int
dsr_gather(nxs_index_t *idx, const void *mine, void *all, size_t len)
{
	if (idx->n_shards <= 1) {
		memcpy(all, mine, len);
		return 0;
	}
	if (nxsgpu_comm_allgather(idx->comm, mine, all, len) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "all-gather failed: %s", nxsgpu_last_error());
		return -1;
	}
	return 0;
}

int
nxs_docshard_refresh_rank(nxs_index_t *shard)
{
	nxs_t *nxs = shard->nxs;
	const unsigned W = shard->n_shards > 1 ? shard->n_shards : 1;
	uint64_t mine[DSR_WORDS], *recs = NULL;
	uint8_t *blk = NULL, *all = NULL;
	uint32_t fin, *fins = NULL;
	size_t len = 0;
	int r, ret = -1;

	nxs_clear_error(nxs);
	if (W > 1 && (!shard->comm || nxsgpu_comm_world(shard->comm) != (int)W ||
	    nxsgpu_comm_rank(shard->comm) != (int)shard->shard)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "shard %u of %u needs a communicator of %u ranks with itself as "
		    "rank %u (nxs_index_shard)", shard->shard, W, W, shard->shard);
		return -1;
	}
	if (pend_oldest(shard)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "batches are in flight");
		return -1;
	}
	recs = malloc((size_t)W * sizeof(mine));
	fins = malloc((size_t)W * sizeof(uint32_t));
	if (!recs || !fins) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	dsr_record(shard, mine);
	if (dsr_gather(shard, mine, recs, sizeof(mine)) != 0) {
		goto fail;
	}
	if ((r = dsr_merge_phase(shard, recs, W, &blk, &len)) <= 0) {
		ret = r;
		goto out;
	}
	if ((all = malloc(len * W)) == NULL) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto fail;
	}
	if (dsr_gather(shard, blk, all, len) != 0) {
		goto fail;
	}
	fin = dsr_finish(shard, all, W, len);
	if (dsr_gather(shard, &fin, fins, sizeof(fin)) != 0) {
		goto fail;
	}
	ret = dsr_settle(shard, fins, W);
	goto out;
fail:
	shard->ds_inconsistent = true;
out:
	free(all);
	free(blk);
	free(recs);
	free(fins);
	return ret;
}

#ifdef NXS_TEST_HOOKS
/*
 * Tests (one GPU, no second rank to talk to): the two halves of the rank form.
 * nxs_test_docshard_block() = this rank's candidate block (malloc'ed);
 * nxs_test_docshard_finish() = what every rank does once it holds all blocks.
 * nxs_test_docshard_set_df() stands in for nxs_docshard_attach()'s collective.
 */
int
nxs_test_docshard_block(nxs_index_t *shard, nxs_params_t *params, const char *const *queries, size_t n,
    uint32_t cap, uint8_t **block, size_t *len)
{
	nxs_index_t *local[1] = { shard };
	nxs_resp_t **resps = calloc(n ? n : 1, sizeof(*resps));
	int r;

	if (!resps) {
		return -1;
	}
	*block = NULL;
	*len = 0;
	r = docshard_search(local, 1, shard->n_shards, shard->shard, params, queries, n,
	    resps, NULL, cap, NULL, block, len, true);
	free(resps);
	return r;
}

int
nxs_test_docshard_finish(nxs_index_t *shard, nxs_params_t *params, const char *const *queries, size_t n,
    uint32_t cap, const uint8_t *gathered, nxs_resp_t **resps, nxs_err_t *errs)
{
	nxs_index_t *local[1] = { shard };

	return docshard_search(local, 1, shard->n_shards, shard->shard, params, queries, n, resps, errs, cap,
	    gathered, NULL, NULL, true);
}

int
nxs_test_docshard_set_df(nxs_index_t *const *shards, unsigned n_shards)
{
	return docshard_set_global_df(shards, n_shards);
}

/*
 * The rank form of nxs_docshard_refresh_rank() with the collectives played by the
 * caller: _record() = this rank's snapshot record, _merge() = agree on the
 * gathered records, walk, merge on the device and hand out this rank's df block
 * (malloc'ed), _finish() = the summed df of the gathered blocks and one impact
 * pass (-> the status this rank reports), _settle() = the outcome of all ranks.
 */
void
nxs_test_docshard_refresh_record(nxs_index_t *shard, uint64_t rec[8])
{
	dsr_record(shard, rec);
}

int
nxs_test_docshard_refresh_merge(nxs_index_t *shard, const uint64_t *recs, unsigned W, uint8_t **block, size_t *len)
{
	nxs_clear_error(shard->nxs);
	return dsr_merge_phase(shard, recs, W, block, len);
}

uint32_t
nxs_test_docshard_refresh_finish(nxs_index_t *shard, const uint8_t *gathered, unsigned W, size_t len)
{
	return dsr_finish(shard, gathered, W, len);
}

int
nxs_test_docshard_refresh_settle(nxs_index_t *shard, const uint32_t *fin, unsigned W)
{
	return dsr_settle(shard, fin, W);
}

/* the snapshot-agreement rule of the rank form (pure host function) */
int
nxs_test_docshard_agree(const uint64_t *recs, unsigned W, const uint64_t consumed[4], uint64_t out[8])
{
	return dsr_agree(recs, W, consumed, out);
}

/* full impact passes of an index's device side so far */
uint64_t
nxs_test_impact_passes(nxs_index_t *idx)
{
	return idx->dev ? nxsgpu_index_impact_passes(idx->dev) : 0;
}

/* total match counts: docs per LDS tile of k_count_tile (byte masks, word masks) */
void
nxs_test_count_tile_widths(uint32_t out[2])
{
	nxsgpu_count_tile_widths(out);
}

#endif /* NXS_TEST_HOOKS */
