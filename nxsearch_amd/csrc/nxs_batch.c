/*
 * nxs_batch.c -- batches between nxs_index_search_batch_begin and _end: the
 * slots in flight, re-sync with the index files, the late second half, queueing
 * on the device, the exact fix-up round and its protocol between the ranks of a
 * query-sharded index, the responses; nxs_index_search[_batch] on top of them.
 *   nxs_index_search      src/query/search.c:285-342
 */
#include <stdlib.h>
#include <string.h>
#include <limits.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"

/* status word of a record slot: 0, an nxs_err_t, or ... */
#define	STATUS_HOSTPATH	0x100u	/* the owner evaluates it on the exact path (fix-up round) */
/*
 * A rank that cannot do its share of a sharded batch (planning failed, out of
 * memory, its exact fix-up failed) must not leave its peers waiting in the
 * all-gather: it still contributes a block, every status word of which carries
 * STATUS_ABORT | its error code.  All ranks see all blocks, so all fail the batch
 * together -- the collectives of every rank stay in step.
 */
#define	STATUS_ABORT	0x200u

/* the first rank whose block says "aborted" (and its error code), or -1 */
static int
blocks_aborted(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k, nxs_err_t *code)
{
	const size_t rec_bytes = NXSGPU_REC_BYTES(k), block_bytes = NXSGPU_BLOCK_BYTES(n_slots, k);

	for (uint32_t r = 0; n_slots && r < world; r++) {
		const uint32_t *st = (const uint32_t *)(blocks + (size_t)r * block_bytes + (size_t)n_slots * rec_bytes);
		if (st[0] & STATUS_ABORT) {
			*code = (nxs_err_t)(st[0] & 0xff);
			return (int)r;
		}
	}
	return -1;
}

nxs_pend_t *
pend_oldest(nxs_index_t *idx)
{
	nxs_pend_t *p = NULL;

	for (int i = 0; i < NXSGPU_INFLIGHT; i++) {
		if (idx->pend[i].active && (!p || idx->pend[i].seq < p->seq)) {
			p = &idx->pend[i];
		}
	}
	return p;
}

static void
pend_release(nxs_pend_t *p)
{
	for (size_t i = 0; p->prep && i < p->hi - p->lo; i++) {
		nxs_query_release(&p->prep[i]);
	}
	free(p->prep);
	for (size_t i = 0; p->xprep && i < p->n; i++) {
		nxs_query_release(&p->xprep[i]);	/* (this rank's slice: never filled) */
	}
	free(p->xprep);
	late_free(p->late);
	for (size_t i = 0; p->st_resps && i < p->n; i++) {
		if (p->st_resps[i]) {		/* stashed and never collected */
			nxs_resp_release(p->st_resps[i]);
		}
	}
	free(p->st_resps);
	free(p->st_errs);
	free(p->st_errmsg);
	memset(p, 0, sizeof(*p));
}

static int batch_end_core(nxs_index_t *, nxs_pend_t *, nxs_resp_t **, nxs_err_t *);

/*
 * search.c:309-312: the reference syncs with the index files before EVERY search.
 * A refresh swaps device arrays the batches in flight read, so when the files
 * have moved (nxs_index_changed: four loads) the batches in flight are finished
 * here, oldest first, their responses kept for the caller's _end -- then the
 * index is refreshed and the new batch sees the change.  In the steady state of
 * a pipelined server (one batch always in flight) nothing else ever would.
 */
/*
 * Finish the batches in flight, oldest first, and keep their outcome (responses, error
 * slot) for the caller's _end.
 */
static int
stash_inflight(nxs_index_t *idx)
{
	int failed = 0;

	(void)late_finish(idx);		/* (a failure is that batch's: kept in its slot) */

	for (;;) {
		nxs_pend_t *pd = NULL;

		for (int i = 0; i < NXSGPU_INFLIGHT; i++) {
			nxs_pend_t *c = &idx->pend[i];
			if (c->active && !c->stashed && (!pd || c->seq < pd->seq)) {
				pd = c;
			}
		}
		if (!pd) {
			if (failed) {
				nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
			}
			return failed;
		}
		pd->st_resps = calloc(pd->n ? pd->n : 1, sizeof(*pd->st_resps));
		pd->st_errs = calloc(pd->n ? pd->n : 1, sizeof(*pd->st_errs));
		if (!pd->st_resps || !pd->st_errs) {
			/*
			 * No memory to keep the batch's outcome: the batch is given up (its _end reports the
			 * error) but its device slot is still handed back HERE, in order -- a caller that goes on
			 * to end a younger slot (abort_collective) must not find this one the oldest.
			 */
			free(pd->st_resps);
			free(pd->st_errs);
			pd->st_resps = NULL;
			pd->st_errs = NULL;
			if (pd->on_device) {
				nxsgpu_batch_view_t v;
				(void)nxsgpu_batch_end(idx->dev, &v);
				pd->on_device = false;
			}
			pd->st_ret = -1;
			pd->st_errcode = NXS_ERR_SYSTEM;
			pd->st_errmsg = strdup("out of memory");
			pd->stashed = true;
			failed = -1;
			continue;
		}
		pd->st_ret = batch_end_core(idx, pd, pd->st_resps, pd->st_errs);
		pd->st_errcode = idx->nxs->errcode;
		pd->st_errmsg = idx->nxs->errmsg ? strdup(idx->nxs->errmsg) : NULL;
		pd->stashed = true;
		nxs_clear_error(idx->nxs);
	}
}

int
resync_before_batch(nxs_index_t *idx)
{
	/*
	 * Sharded: the fix-up round of a batch in flight is a collective, so the ranks have to
	 * agree on WHICH _begin finishes the batches in flight.  Each rank says in the flags
	 * word of its record block whether it saw the files move (NXSGPU_BLOCK_CHANGED, set in
	 * _begin); every rank reads all flags after the all-gather (batch_end_core) and, if any
	 * is set, drains at its next _begin -- the same one on every rank, since all of them
	 * make the same calls in the same order.
	 */
	if (pend_oldest(idx)) {
		if (idx->comm ? !idx->resync_pending : !nxs_index_changed(idx)) {
			return idx->comm ? 0 : nxs_index_refresh(idx);
		}
		if (stash_inflight(idx) == -1) {
			return -1;
		}
	}
	idx->resync_pending = false;
	return nxs_index_refresh(idx);
}

/* any rank's block flags say "my index files moved" (all W blocks present) */
static bool
blocks_changed(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k)
{
	const size_t rec_bytes = NXSGPU_REC_BYTES(k), block_bytes = NXSGPU_BLOCK_BYTES(n_slots, k);

	for (uint32_t r = 0; r < world; r++) {
		const uint32_t *st = (const uint32_t *)(blocks + (size_t)r * block_bytes + (size_t)n_slots * rec_bytes);
		if (st[n_slots] & NXSGPU_BLOCK_CHANGED) {
			return true;
		}
	}
	return false;
}

/* batches never collected (the caller closes the index instead): wait, drop */
void
index_drain(nxs_index_t *idx)
{
	nxs_pend_t *pd;

	if (idx->dev) {
		(void)late_finish(idx);
	}
	while ((pd = pend_oldest(idx)) != NULL) {
		nxsgpu_batch_view_t v;

		if (pd->on_device && !pd->stashed && idx->dev) {
			(void)nxsgpu_batch_end(idx->dev, &v);
		}
		pend_release(pd);
	}
}

/* the planned batch (record path: limit <= NXSGPU_BIG_K) onto the device; 0, or -1 with the error declared */
static int
queue_on_device(nxs_index_t *idx, nxs_pend_t *pd, const search_params_t *sp, bool collective)
{
	nxs_t *nxs = idx->nxs;
	const size_t nl = pd->hi - pd->lo;
	nxsgpu_query_t *plans = malloc((nl ? nl : 1) * sizeof(nxsgpu_query_t));
	uint32_t *slot_of = malloc((nl ? nl : 1) * sizeof(uint32_t));
	uint32_t *status = calloc(NXSGPU_STATUS_WORDS(pd->cap), sizeof(uint32_t));
	size_t n_plans = 0;
	int ret = -1;

	if (!plans || !slot_of || !status) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	for (size_t i = 0; i < nl; i++) {
		const qprep_t *q = &pd->prep[i];

		if (q->errcode) {
			status[i] = q->errcode;
		} else if (q->wide) {
			status[i] = STATUS_HOSTPATH;
		} else if (!q->empty) {
			slot_of[n_plans] = (uint32_t)i;
			plans[n_plans++] = q->plan;
		}
	}
	if (collective && nxs_index_changed(idx)) {
		/* a batch is in flight (else resync_before_batch refreshed just now): tell
		 * the peers, all ranks drain and re-sync together */
		status[pd->cap] = NXSGPU_BLOCK_CHANGED;
	}
	/* the worker threads are lent for THIS call only (the pool takes one run at a time: the doc-shard
	 * entry runs a host thread per shard through the same device layer and must never find it set) */
	nxsgpu_index_set_parallel(idx->dev, api_parallel, nxs);
	const nxsgpu_batch_opts_t bo = { .totals = pd->want_total };
	const int brc = nxsgpu_batch_begin_opts(idx->dev, sp->algo, (uint32_t)sp->limit, plans,
	    (uint32_t)n_plans, slot_of, status, pd->cap,
	    idx->comm != NULL && pd->world >= 1 && !idx->emu_world, pd->want_total ? &bo : NULL);
	nxsgpu_index_set_parallel(idx->dev, NULL, NULL);
	if (brc != 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "device search failed: %s", nxsgpu_last_error());
		goto out;
	}
	pd->on_device = true;
	ret = 0;
out:
	free(plans);
	free(slot_of);
	free(status);
	return ret;
}

/*
 * The second half of a batch whose fuzzy pass was left running (struct late_half), in two steps: COLLECT
 * waits for the pass and takes its winners (the fuzzy workspaces are free again: the next batch's pass can
 * be queued), COMPLETE finishes the plans and queues the batch.  The batch's _begin has long returned
 * success, so a failure here is kept in the batch's slot for its _end (like a batch finished early by a
 * re-sync).
 */
static nxs_pend_t *
late_oldest(nxs_index_t *idx)
{
	nxs_pend_t *pd = NULL;

	for (int i = 0; i < NXSGPU_INFLIGHT; i++) {
		nxs_pend_t *c = &idx->pend[i];
		if (c->active && c->late && (!pd || c->seq < pd->seq)) {
			pd = c;
		}
	}
	return pd;
}

static void
late_failed(nxs_index_t *idx, nxs_pend_t *pd)
{
	nxs_t *nxs = idx->nxs;

	pd->st_ret = -1;
	pd->st_errcode = nxs->errcode ? nxs->errcode : NXS_ERR_FATAL;
	pd->st_errmsg = nxs->errmsg ? strdup(nxs->errmsg) : NULL;
	pd->stashed = true;
	nxs_clear_error(nxs);
	late_free(pd->late);
	pd->late = NULL;
}

static int
late_collect(nxs_index_t *idx, nxs_pend_t *pd)
{
	struct late_half *lh = pd->late;
	const double t0 = now_s();

	if (lh->collected) {
		return 0;
	}
	if (nxsgpu_fuzzy_end(idx->dev, lh->slot, lh->fz.bytes, lh->fz.off, (uint32_t)lh->fz.n, lh->fz.ids) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "device fuzzy search failed: %s", nxsgpu_last_error());
		late_failed(idx, pd);
		return -1;
	}
	lh->collected = true;
	idx->hp_fzwait += now_s() - t0;
	idx->hp_plan += now_s() - t0;
	return 0;
}

static int
late_complete(nxs_index_t *idx, nxs_pend_t *pd)
{
	struct late_half *lh = pd->late;
	const double t0 = now_s();
	double t1;

	plan_back(idx, &lh->sp, lh->queries, pd->hi - pd->lo, pd->prep, &lh->fz);
	t1 = now_s();
	idx->hp_back += t1 - t0;
	idx->hp_plan += t1 - t0;
	if ((idx->test_fail_late && idx->test_fail_late-- == 1 &&
	    (nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "injected failure in the late half (test)"), true)) ||
	    queue_on_device(idx, pd, &lh->sp, false) != 0) {
		late_failed(idx, pd);
		return -1;
	}
	idx->hp_queue += now_s() - t1;
	late_free(lh);
	pd->late = NULL;
	return 0;
}

/* every late batch, oldest first (0: nothing to do, or all went well) */
int
late_finish(nxs_index_t *idx)
{
	nxs_pend_t *pd;
	int ret = 0;

	while ((pd = late_oldest(idx)) != NULL) {
		if (late_collect(idx, pd) != 0 || late_complete(idx, pd) != 0) {
			ret = -1;
		}
	}
	return ret;
}

/*
 * The body of a _begin, after the params have been read.  The batch is n query strings -- or, docs != NULL
 * (queries is NULL then), nxs_index_similar's: query i is the doc leaf of docs[i], resolved with the batch's
 * other docs in plan_front; such a batch has no fuzzy misses and is never left with a late half.
 */
static int
batch_begin(nxs_index_t *idx, const search_params_t *spp, const char *const *queries, const nxs_doc_id_t *docs, size_t n)
{
	nxs_t *nxs = idx->nxs;
	nxs_pend_t *pd = NULL;
	const search_params_t sp = *spp;
	uint32_t *status = NULL;
	uint64_t lo = 0, hi = n;
	size_t nl;
	double t0, t1 = 0;
	const double t_in = now_s();
	fz_set_t fz = { 0 };
	nxs_pend_t *old;
	int ret = -1;

	/* (totals would have to travel in the record blocks all ranks agree on: a follow-up, include/nxs.h;
	 * every rank passes the same params, so every rank refuses) */
	if (sp.total && (idx->comm || idx->emu_world > 1)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "total is not available on a sharded batch");
		return -1;
	}
	for (int i = 0; i < NXSGPU_INFLIGHT; i++) {
		if (!idx->pend[i].active) {
			pd = &idx->pend[i];
			break;
		}
	}
	if (!pd) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "%d batches are already in flight", NXSGPU_INFLIGHT);
		return -1;
	}
	/* search.c:309-312: pick up what other processes appended or removed */
	if (resync_before_batch(idx) == -1) {
		return -1;
	}
	if (n > UINT32_MAX / 2) {
		nxs_decl_err(nxs, NXS_ERR_LIMIT, "batch too large");
		return -1;
	}
	memset(pd, 0, sizeof(*pd));
	pd->n = n;
	pd->limit = sp.limit;
	pd->algo = sp.algo;
	pd->want_total = sp.total;
	pd->want_explain = sp.explain;
	pd->world = 1;
	/* query sharding: fixed-size records, limit <= NXSGPU_BIG_K;
	 * larger limits run replicated -- every rank computes the whole batch */
	if (idx->comm && sp.limit <= NXSGPU_BIG_K) {
		pd->rank = nxsgpu_comm_rank(idx->comm);
		pd->world = nxsgpu_comm_world(idx->comm);
		nxsgpu_shard_slice(n, pd->rank, pd->world, &lo, &hi);
	} else if (idx->emu_world > 1 && sp.limit <= NXSGPU_BIG_K) {
		/* tests: this process plays ONE rank of a W-rank run, no collective */
		pd->rank = idx->emu_rank;
		pd->world = idx->emu_world;
		nxsgpu_shard_slice(n, pd->rank, pd->world, &lo, &hi);
	}
	pd->lo = lo;
	pd->hi = hi;
	pd->cap = (uint32_t)nxsgpu_shard_capacity(n, pd->world);
	nl = hi - lo;
	/* (a rank of a real communicator: its peers queue an all-gather for this batch, so from
	 * here on a failure of this rank still has to contribute a block: abort_collective) */
	const bool collective = idx->comm != NULL && !idx->emu_world && sp.limit <= NXSGPU_BIG_K;
	pd->prep = calloc(nl ? nl : 1, sizeof(qprep_t));
	if (!pd->prep) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		if (collective) {
			goto abort_collective;
		}
		goto out;
	}
	t0 = now_s();
	if (plan_front(idx, &sp, queries ? queries + lo : NULL, docs ? docs + lo : NULL, nl, pd->prep, &fz) == -1 ||
	    (idx->test_fail_begin && idx->test_fail_begin-- == 1 &&
	    (nxs_decl_err(nxs, NXS_ERR_SYSTEM, "injected failure (test)"), true))) {
		(void)late_finish(idx);
		if (collective) {
			goto abort_collective;
		}
		goto out;
	}
	t1 = now_s();
	idx->hp_front += t1 - t0;
	idx->hp_plan += t1 - t0;
	/*
	 * The batch before this one may still lack its second half: its fuzzy pass has had the time since its
	 * _begin returned (the caller's work, this batch's parse).  THIS batch's pass is queued first (the
	 * device layer has two sets of fuzzy workspaces; the passes run in order), then the older batch's
	 * winners are collected, its plans compiled and the batch sent to the device -- it still goes there
	 * before this one.  A failure of the older batch is its own (reported by its _end).
	 */
	old = late_oldest(idx);
	t0 = now_s();
	if (fz.n) {
		if (!idx->late_mode) {
			const char *e = getenv("NXS_LATE_FUZZY");	/* (once per index: the query path reads no environment) */
			idx->late_mode = e && atoi(e) == 0 ? 2 : 1;
		}
		/* (sharded batches, doc shards and limits beyond the record path wait for the pass here: their
		 * failure paths are collectives of their own) */
		const bool late = idx->late_mode == 1 && !collective && !idx->comm && !idx->emu_world &&
		    !idx->n_shards && sp.limit <= NXSGPU_BIG_K;
		struct late_half *lh = NULL;
		bool failed;

		if (old && (!late || idx->bk_upto != idx->last_id || idx->bk_flags_stale)) {
			/* (the BK-tree image is about to be replaced, or this batch's pass runs at once:
			 * nothing of the older batch's may be on the device then) */
			(void)late_finish(idx);
			old = NULL;
			t0 = now_s();
		}
		failed = nxs_index_bk_sync(idx) == -1;
		if (!failed && late) {
			if ((lh = late_make(&sp, &fz, queries + lo, nl, pd->prep)) == NULL) {
				nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
				failed = true;
			} else if ((lh->slot = nxsgpu_fuzzy_begin(idx->dev, lh->fz.bytes, lh->fz.off, (uint32_t)lh->fz.n)) < 0) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "device fuzzy search failed: %s", nxsgpu_last_error());
				late_free(lh);
				lh = NULL;
				failed = true;
			}
		}
		idx->hp_fzlaunch += now_s() - t0;
		idx->hp_plan += now_s() - t0;
		if (old) {
			/* (its failure would wipe this batch's error slot: kept aside) */
			const nxs_err_t code = nxs->errcode;
			char *msg = failed && nxs->errmsg ? strdup(nxs->errmsg) : NULL;

			if (late_collect(idx, old) == 0) {
				(void)late_complete(idx, old);
			}
			old = NULL;
			if (failed) {
				nxs_decl_err(nxs, code ? code : NXS_ERR_FATAL, "%s", msg ? msg : "");
			}
			free(msg);
		}
		if (failed) {
			if (collective) {
				goto abort_collective;
			}
			goto out;
		}
		if (lh) {
			pd->late = lh;
			idx->hp_batches++;
			idx->hp_begin += now_s() - t_in;
			pd->seq = ++idx->pend_seq;
			pd->active = true;
			ret = 0;
			goto out;
		}
		t0 = now_s();
		if (nxsgpu_fuzzy(idx->dev, fz.bytes, fz.off, (uint32_t)fz.n, fz.ids, NULL) != 0) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "device fuzzy search failed: %s", nxsgpu_last_error());
			if (collective) {
				goto abort_collective;
			}
			goto out;
		}
		idx->hp_fzwait += now_s() - t0;
	}
	if (old && late_collect(idx, old) == 0) {
		(void)late_complete(idx, old);
	}
	t1 = now_s();
	plan_back(idx, &sp, queries ? queries + lo : NULL, nl, pd->prep, &fz);
	idx->hp_back += now_s() - t1;
	if (sp.explain && pd->world > 1 && !idx->shard_local) {
		/*
		 * This rank will hold every response of the batch and explains them all from its replica, with no
		 * collective: it needs the token lists of the other ranks' queries too.  Every replica has the same
		 * dictionary, so planning them here yields what their owners planned.  (Sharded batches never leave
		 * a fuzzy pass running: plan_batch's blocking pass is the only one.)
		 */
		pd->xprep = calloc(n ? n : 1, sizeof(qprep_t));
		if (!pd->xprep) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		}
		if (!pd->xprep || (lo && plan_batch(idx, &sp, queries, docs, lo, pd->xprep) == -1) ||
		    (hi < n && plan_batch(idx, &sp, queries ? queries + hi : NULL, docs ? docs + hi : NULL, n - hi,
		    pd->xprep + hi) == -1)) {
			if (collective) {
				goto abort_collective;
			}
			goto out;
		}
	}
	t1 = now_s();
	idx->hp_plan += t1 - t0;
	if (sp.limit <= NXSGPU_BIG_K) {
		const int qrc = queue_on_device(idx, pd, &sp, collective);

		if (qrc != 0) {
			if (collective) {
				goto abort_collective;	/* (an empty block may still go up) */
			}
			goto out;
		}
	}
	idx->hp_queue += now_s() - t1;
	idx->hp_batches++;
	idx->hp_begin += now_s() - t_in;
	pd->seq = ++idx->pend_seq;
	pd->active = true;
	ret = 0;
out:
	fz_set_free(&fz);
	free(status);
	if (ret != 0) {
		pend_release(pd);
	}
	return ret;

abort_collective:
	/*
	 * This rank cannot do its share, but its peers have queued (or will queue) the
	 * batch's all-gather: contribute a block that says so and wait for the
	 * collective, so that every rank fails this batch and the next one starts in
	 * step.  The error of this rank stays in its slot.
	 */
	{
		const nxs_err_t code = nxs->errcode ? nxs->errcode : NXS_ERR_FATAL;
		char *msg = nxs->errmsg ? strdup(nxs->errmsg) : NULL;
		nxsgpu_batch_view_t v;

		free(status);
		status = calloc(NXSGPU_STATUS_WORDS(pd->cap), sizeof(uint32_t));
		for (uint32_t i = 0; status && i < pd->cap; i++) {
			status[i] = STATUS_ABORT | (uint32_t)code;
		}
		/*
		 * Order: the block's all-gather is queued FIRST (the peers queued theirs in their
		 * _begin), then the batches this rank still has in flight are finished -- the
		 * device hands its slots back oldest first, and an older batch's fix-up round is
		 * a collective the peers enter in their _end, after this batch's all-gather --,
		 * their outcome kept for the caller's _end; only then is the abort slot the
		 * oldest one.  (Ending it at once took the OLDER batch's slot: that batch's
		 * _end then read the abort block as its own.)
		 */
		if (nxsgpu_batch_begin(idx->dev, sp.algo, (uint32_t)sp.limit, NULL, 0, NULL, status, pd->cap, 1) == 0) {
			(void)stash_inflight(idx);
			(void)nxsgpu_batch_end(idx->dev, &v);
		}
		/* (if even the empty block cannot go up the communicator is unusable: the peers'
		 * collective never completes -- fatal for the sharded group) */
		nxs_decl_err(nxs, code, "%s", msg ? msg : "this rank aborted the sharded batch");
		free(msg);
	}
	goto out;
}

int
nxs_index_search_batch_begin(nxs_index_t *idx, nxs_params_t *params,
    const char *const *queries, size_t n)
{
	search_params_t sp;

	nxs_clear_error(idx->nxs);
	if (get_search_params(idx, params, &sp) == -1) {
		return -1;
	}
	return batch_begin(idx, &sp, queries, NULL, n);
}

/* exact path (nxsgpu_search / nxsgpu_search_wide) for the given local queries */
/*
 * tot (or NULL): the total match count of every such query, [nw] -- what the exact path's own count pass
 * matched.  Fixed-size plans at a limit the candidate filter serves (the re-runs of a record batch's overflowed
 * queries) are NOT counted again: the batch's count kernels have counted them, tot[j] stays TOT_KEEP.
 */
#define	TOT_KEEP	UINT64_MAX
static int
run_exact(nxs_index_t *idx, const nxs_pend_t *pd, const uint32_t *which, size_t nw,
    nxsgpu_results_t *res, nxsgpu_results_t *wres, uint32_t *pos, uint64_t *tot)
{
	nxsgpu_query_t *plans = NULL;
	nxsgpu_wide_query_t *wplans = NULL;
	uint32_t *t32 = NULL, *w32 = NULL;
	const bool all_exact = pd->limit > NXSGPU_BIG_K;
	size_t np = 0, nwd = 0;
	int ret = -1;

	memset(res, 0, sizeof(*res));
	memset(wres, 0, sizeof(*wres));
	plans = malloc((nw ? nw : 1) * sizeof(nxsgpu_query_t));
	wplans = malloc((nw ? nw : 1) * sizeof(nxsgpu_wide_query_t));
	if (!plans || !wplans) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	for (size_t j = 0; j < nw; j++) {
		const qprep_t *q = &pd->prep[which[j]];

		if (q->wide) {
			pos[j] = (uint32_t)nwd | 0x80000000u;
			wplans[nwd++] = q->wplan;
		} else {
			pos[j] = (uint32_t)np;
			plans[np++] = q->plan;
		}
	}
	if (tot) {
		t32 = calloc(np ? np : 1, sizeof(uint32_t));
		w32 = calloc(nwd ? nwd : 1, sizeof(uint32_t));
		if (!t32 || !w32) {
			nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
			goto out;
		}
	}
	if (np && ((tot && all_exact) ?
	    nxsgpu_search_totals(idx->dev, pd->algo, pd->limit, plans, (uint32_t)np, res, t32) :
	    nxsgpu_search(idx->dev, pd->algo, pd->limit, plans, (uint32_t)np, res)) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "device search failed: %s", nxsgpu_last_error());
		goto out;
	}
	if (nwd && (tot ? nxsgpu_search_wide_totals(idx->dev, pd->algo, pd->limit, wplans, (uint32_t)nwd, wres, w32) :
	    nxsgpu_search_wide(idx->dev, pd->algo, pd->limit, wplans, (uint32_t)nwd, wres)) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "device search failed: %s", nxsgpu_last_error());
		goto out;
	}
	for (size_t j = 0; tot && j < nw; j++) {
		tot[j] = (pos[j] & 0x80000000u) ? w32[pos[j] & 0x7fffffffu] : all_exact ? t32[pos[j]] : TOT_KEEP;
	}
	ret = 0;
out:
	free(plans);
	free(wplans);
	free(t32);
	free(w32);
	return ret;
}

static inline const nxsgpu_results_t *
exact_pick(const nxsgpu_results_t *res, const nxsgpu_results_t *wres, uint32_t pos, uint32_t *at)
{
	*at = pos & 0x7fffffffu;
	return (pos & 0x80000000u) ? wres : res;
}

/*
 * Responses of a whole batch from the ranks' record blocks, in query order
 * (rank r owns the contiguous slice nxsgpu_shard_slice(n, r, world)).  A slot
 * with a status word is a failed query: no response, its code in errs[].
 */
static int
resps_from_blocks(nxs_t *nxs, const nxs_pend_t *pd, size_t n, uint32_t world, uint32_t n_slots,
    uint32_t k, const uint8_t *blocks, nxs_resp_t **resps, nxs_err_t *errs, slab_builder_t *sb,
    int *failed, int only_rank)
{
	const size_t rec_bytes = NXSGPU_REC_BYTES(k), block_bytes = NXSGPU_BLOCK_BYTES(n_slots, k);
	size_t total = 0;

	/* only_rank >= 0 (nxs_index_shard_local): that rank's slice alone -- the other slices' responses stay
	 * NULL and their errs[] untouched: O(n / world) host work per rank and batch instead of O(n) */
	for (uint32_t r = 0; r < world; r++) {
		const uint8_t *blk = blocks + (size_t)r * block_bytes;
		uint64_t rlo, rhi;

		if (only_rank >= 0 && (int)r != only_rank) {
			continue;
		}
		nxsgpu_shard_slice(n, (int)r, (int)world, &rlo, &rhi);
		for (uint64_t i = 0; i < rhi - rlo; i++) {
			const uint32_t c = ((const uint32_t *)(blk + i * rec_bytes))[0];
			if (c > k) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "corrupted result record");
				return -1;
			}
			total += c;
		}
	}
	if (slab_begin(sb, n, total) == -1) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		return -1;
	}
	for (uint32_t r = 0; r < world; r++) {
		const uint8_t *blk = blocks + (size_t)r * block_bytes;
		const uint32_t *st = (const uint32_t *)(blk + (size_t)n_slots * rec_bytes);
		uint64_t rlo, rhi;

		if (only_rank >= 0 && (int)r != only_rank) {
			continue;
		}
		nxsgpu_shard_slice(n, (int)r, (int)world, &rlo, &rhi);
		for (uint64_t i = 0; i < rhi - rlo; i++) {
			const uint8_t *rec = blk + i * rec_bytes;
			const uint32_t c = ((const uint32_t *)rec)[0];
			nxs_resp_t *rp;

			if (st[i]) {
				(*failed)++;
				if (errs) {
					errs[rlo + i] = (nxs_err_t)st[i];
				}
				if (pd && (int)r == pd->rank) {
					nxs_decl_err(nxs, (nxs_err_t)st[i], "%s",
					    pd->prep[i].errmsg ? pd->prep[i].errmsg : "");
				} else {
					nxs_decl_err(nxs, (nxs_err_t)st[i], "query %llu failed on rank %u",
					    (unsigned long long)(rlo + i), r);
				}
				continue;
			}
			rp = slab_resp(sb, rlo + i, c);
			memcpy(rp->ids, rec + 8, (size_t)c * 8);
			memcpy(rp->scores, rec + 8 + 8 * (size_t)k, (size_t)c * 4);
			resps[rlo + i] = rp;
		}
	}
	return 0;
}

int
nxs_index_search_batch_end(nxs_index_t *idx, nxs_resp_t **resps, nxs_err_t *errs)
{
	nxs_pend_t *pd = pend_oldest(idx);
	int ret;

	if (!pd) {
		nxs_clear_error(idx->nxs);
		nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "no batch in flight");
		return -1;
	}
	if (pd->late) {
		(void)late_finish(idx);		/* (no later _begin came by: the second half runs here) */
	}
	if (pd->stashed) {
		/* finished early by a later _begin (resync_before_batch): hand over */
		nxs_clear_error(idx->nxs);
		for (size_t i = 0; i < pd->n; i++) {
			resps[i] = pd->st_resps ? pd->st_resps[i] : NULL;
			if (pd->st_resps) {
				pd->st_resps[i] = NULL;
			}
			if (errs) {
				errs[i] = pd->st_errs ? pd->st_errs[i] : pd->st_errcode;
			}
		}
		if (pd->st_errcode) {
			nxs_decl_err(idx->nxs, pd->st_errcode, "%s", pd->st_errmsg ? pd->st_errmsg : "");
		}
		ret = pd->st_ret;
	} else {
		ret = batch_end_core(idx, pd, resps, errs);
	}
	pend_release(pd);
	return ret;
}

/*
 * The fix-up round of a sharded batch, as every rank decides it from the gathered blocks:
 * a record marked inexact (candidate overflow) or a host-path query (wide plan) anywhere
 * means ALL ranks take a second all-gather, after each owner has re-run its own such
 * queries on the exact path (`which`: the owner's, local indexes).  `all` = the blocks of
 * all W ranks are present (else: this rank's block only -- one emulated rank, tests).
 */
static bool
fixup_scan(const uint8_t *blocks, bool all, uint32_t W, int rank, uint32_t n_slots, uint32_t k,
    size_t n, uint32_t *which, size_t *nw)
{
	const size_t rec_bytes = NXSGPU_REC_BYTES(k), block_bytes = NXSGPU_BLOCK_BYTES(n_slots, k);
	bool fixup = false;

	for (uint32_t r = 0; r < W; r++) {
		const uint8_t *blk = all ? blocks + (size_t)r * block_bytes : blocks;
		const uint32_t *st = (const uint32_t *)(blk + (size_t)n_slots * rec_bytes);
		uint64_t rlo, rhi;

		if (!all && (int)r != rank) {
			continue;
		}
		nxsgpu_shard_slice(n, (int)r, (int)W, &rlo, &rhi);
		for (uint64_t i = 0; i < rhi - rlo; i++) {
			const uint32_t *rec = (const uint32_t *)(blk + i * rec_bytes);
			if (rec[1] == NXSGPU_REC_INEXACT || st[i] == STATUS_HOSTPATH) {
				fixup = true;
				if ((int)r == rank) {
					which[(*nw)++] = (uint32_t)i;
				}
			}
		}
	}
	return fixup;
}

/* after the second all-gather: the rank that aborted in the fix-up round, or one that left a
 * record unpatched (still marked) -- every rank fails the batch then --, else -1 */
static int
fixup_verify(const uint8_t *blocks, uint32_t W, uint32_t n_slots, uint32_t k, size_t n, nxs_err_t *acode)
{
	const size_t rec_bytes = NXSGPU_REC_BYTES(k), block_bytes = NXSGPU_BLOCK_BYTES(n_slots, k);
	int ar = blocks_aborted(blocks, W, n_slots, k, acode);

	for (uint32_t r = 0; ar < 0 && r < W; r++) {
		const uint8_t *blk = blocks + (size_t)r * block_bytes;
		const uint32_t *st = (const uint32_t *)(blk + (size_t)n_slots * rec_bytes);
		uint64_t rlo, rhi;

		nxsgpu_shard_slice(n, (int)r, (int)W, &rlo, &rhi);
		for (uint64_t i = 0; i < rhi - rlo; i++) {
			if (((const uint32_t *)(blk + i * rec_bytes))[1] == NXSGPU_REC_INEXACT || st[i] == STATUS_HOSTPATH) {
				ar = (int)r;
				*acode = NXS_ERR_FATAL;
			}
		}
	}
	return ar;
}

/*
 * "explain": every response of the batch that this rank holds gets its explanation, from this rank's device
 * index, in one pass.  Called where the responses are materialised (batch_end_core -- also for a batch that
 * a later _begin finishes early because the files moved: the explanation belongs to the snapshot the results
 * came from, and the device index has not moved yet).  The slice [lo, hi) has its plans in pd->prep, the
 * other ranks' queries (all blocks gathered, own-slice mode off) in pd->xprep.
 */
static int
explain_batch(nxs_index_t *idx, const nxs_pend_t *pd, nxs_resp_t **resps, struct resp_slab *slab)
{
	nxs_index_t *one[1] = { idx };
	ex_item_t *items = malloc((pd->n ? pd->n : 1) * sizeof(ex_item_t));
	size_t ni = 0;
	int ret;

	if (!items) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
		return -1;
	}
	for (size_t i = 0; i < pd->n; i++) {
		const bool mine = i >= pd->lo && i < pd->hi;
		const qprep_t *q = mine ? &pd->prep[i - pd->lo] : pd->xprep ? &pd->xprep[i] : NULL;

		if (!resps[i]) {
			continue;
		}
		resps[i]->explained = true;
		if (!q || q->errcode || q->empty || !resps[i]->count) {
			if (!q && resps[i]->count) {
				nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "explain: no plan for query %zu", i);
				free(items);
				return -1;
			}
			continue;
		}
		ex_item_of(&items[ni++], resps[i], q);
	}
	ret = explain_attach(one, 1, pd->algo, items, ni, slab);
	free(items);
	return ret;
}

static int
batch_end_core(nxs_index_t *idx, nxs_pend_t *pd, nxs_resp_t **resps, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	nxsgpu_results_t res, wres;
	slab_builder_t sb = { 0 };
	uint8_t *patched = NULL;
	bool patched_own = true;	/* `patched` is malloc()ed (not the slot's pinned blocks) */
	uint32_t *which, *pos;
	uint64_t *tot = NULL, *xtot = NULL;	/* want_total: per local query / per exact re-run */
	size_t nw = 0, total = 0, n, nl;
	double t0;
	const double t_in = now_s();
	int failed = 0, ret = -1;

	memset(&res, 0, sizeof(res));
	memset(&wres, 0, sizeof(wres));
	nxs_clear_error(nxs);
	n = pd->n;
	nl = pd->hi - pd->lo;
	outs_clear(resps, errs, n);
	which = calloc(nl ? nl : 1, sizeof(uint32_t));
	pos = calloc(nl ? nl : 1, sizeof(uint32_t));
	if (pd->want_total) {
		/* (never sharded: the slice is the whole batch) */
		tot = calloc(nl ? nl : 1, sizeof(uint64_t));
		xtot = calloc(nl ? nl : 1, sizeof(uint64_t));
	}
	if (!which || !pos || (pd->want_total && (!tot || !xtot))) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}

	if (pd->on_device) {
		nxsgpu_batch_view_t v;
		const uint32_t *dev_tot = NULL;
		const uint8_t *blocks;
		const uint32_t W = (uint32_t)pd->world;
		/* all W blocks are present after the all-gather; a single rank -- or the
		 * emulation of one rank of W (tests) -- holds its own block only */
		const bool all = W == 1 || !idx->emu_world;
		bool fixup = false;

		t0 = now_s();
		if (nxsgpu_batch_end_totals(idx->dev, &v, &dev_tot) != 0) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "device search failed: %s", nxsgpu_last_error());
			goto out;
		}
		idx->hp_wait += now_s() - t0;
		if (tot) {
			/* the device's totals are in plan order: the queries queue_on_device sent */
			size_t j = 0;
			for (size_t i = 0; i < nl; i++) {
				const qprep_t *q = &pd->prep[i];
				if (!q->errcode && !q->wide && !q->empty) {
					if (!dev_tot) {
						nxs_decl_err(nxs, NXS_ERR_FATAL, "the batch came back without its totals");
						goto out;
					}
					tot[i] = dev_tot[j++];
				}
			}
		}
		t0 = now_s();
		blocks = v.blocks;
		if (all && v.world != W) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "sharded batch came back with %u blocks, not %u",
			    v.world, W);
			goto out;
		}
		if (all && idx->comm && blocks_changed(blocks, W, v.n_slots, v.k)) {
			idx->resync_pending = true;	/* (every rank reads the same flags) */
		}
		if (all) {
			nxs_err_t acode;
			const int ar = blocks_aborted(blocks, W, v.n_slots, v.k, &acode);
			if (ar >= 0) {
				/* every rank sees it: all of them fail here, none enters a fix-up round */
				nxs_decl_err(nxs, acode ? acode : NXS_ERR_FATAL, "rank %d aborted the sharded batch", ar);
				goto out;
			}
		}
		/* records that need the exact path: every rank sees the same flags, so
		 * every rank takes (or skips) the fix-up round together */
		fixup = fixup_scan(blocks, all, W, pd->rank, v.n_slots, v.k, n, which, &nw);
		if (fixup) {
			const size_t len = (all ? (size_t)W : 1) * v.block_bytes;
			uint8_t *mine;

			bool fix_failed = false;
			char *fix_msg = NULL;
			nxs_err_t fix_code = NXS_ERR_SUCCESS;

			if ((patched = malloc(len ? len : 1)) == NULL) {
				nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
				if (!(all && W > 1)) {
					goto out;
				}
				/* (the peers are on their way into the fix-up all-gather: send the
				 * unpatched block -- records still marked inexact fail the batch on
				 * every rank, below) */
				fix_failed = true;
				fix_code = NXS_ERR_SYSTEM;
			} else {
				memcpy(patched, blocks, len);
			}
			mine = patched ? patched + (all ? (size_t)pd->rank * v.block_bytes : 0) :
			    (uint8_t *)(uintptr_t)(blocks + (size_t)pd->rank * v.block_bytes);
			if (!fix_failed && (run_exact(idx, pd, which, nw, &res, &wres, pos, xtot) != 0 ||
			    (idx->test_fail_fixup && idx->test_fail_fixup-- == 1 &&
			    (nxs_decl_err(nxs, NXS_ERR_SYSTEM, "injected failure (test)"), true)))) {
				if (!(all && W > 1)) {
					goto out;
				}
				/* this rank's exact pass failed: say so in its block and still take
				 * part in the collective */
				uint32_t *st = (uint32_t *)(mine + (size_t)v.n_slots * v.rec_bytes);
				fix_failed = true;
				fix_code = nxs->errcode ? nxs->errcode : NXS_ERR_FATAL;
				fix_msg = nxs->errmsg ? strdup(nxs->errmsg) : NULL;
				for (uint32_t i = 0; i < v.n_slots; i++) {
					st[i] = STATUS_ABORT | (uint32_t)fix_code;
				}
			}
			idx->hp_inexact += nw;
			for (size_t j = 0; !fix_failed && j < nw; j++) {
				uint8_t *rec = mine + (size_t)which[j] * v.rec_bytes;
				uint32_t *st = (uint32_t *)(mine + (size_t)v.n_slots * v.rec_bytes);
				uint32_t at;
				const nxsgpu_results_t *rs = exact_pick(&res, &wres, pos[j], &at);
				const uint32_t c = rs->counts[at];

				((uint32_t *)rec)[0] = c;
				((uint32_t *)rec)[1] = 0;
				memcpy(rec + 8, rs->doc_ids + rs->offsets[at], (size_t)c * 8);
				memcpy(rec + 8 + 8 * (size_t)v.k, rs->scores + rs->offsets[at], (size_t)c * 4);
				st[which[j]] = 0;
				if (tot && xtot[j] != TOT_KEEP) {
					tot[which[j]] = xtot[j];	/* (wide plans: k_scanw's count pass; the others were counted with the batch) */
				}
			}
			if (all && W > 1) {
				uint8_t *gathered = malloc(len);
				bool g_own = gathered != NULL;

				/*
				 * No memory to receive into: the slot's own pinned blocks (the first
				 * round's result: W blocks, the size this round needs) are always
				 * there -- the all-gather stages through device memory, so receiving
				 * over the block that is being sent is safe -- and what this rank
				 * needs of the first round is in `patched` (or it sends its block
				 * unpatched, which fails the batch everywhere).  A rank that is out
				 * of memory no longer strands its peers.
				 */
				if (!gathered || (idx->test_fail_fixup_recv && idx->test_fail_fixup_recv-- == 1)) {
					free(gathered);
					gathered = (uint8_t *)(uintptr_t)v.blocks;
					g_own = false;
				}
				if (nxsgpu_comm_allgather(idx->comm, mine, gathered, v.block_bytes) != 0) {
					nxs_decl_err(nxs, NXS_ERR_FATAL, "all-gather failed: %s", nxsgpu_last_error());
					if (g_own) {
						free(gathered);
					}
					free(fix_msg);
					goto out;
				}
				free(patched);
				patched = gathered;
				patched_own = g_own;
				{
					nxs_err_t acode;
					const int ar = fixup_verify(patched, W, v.n_slots, v.k, n, &acode);
					if (ar >= 0) {
						if (ar == pd->rank && fix_code) {
							nxs_decl_err(nxs, fix_code, "%s", fix_msg ? fix_msg : "exact pass failed");
						} else {
							nxs_decl_err(nxs, acode ? acode : NXS_ERR_FATAL,
							    "rank %d aborted the sharded batch (exact fix-up round)", ar);
						}
						free(fix_msg);
						goto out;
					}
				}
			}
			free(fix_msg);
			blocks = patched;
		}
		if (!all) {
			/* one rank of an emulated W-rank run: hand the block to the test */
			free(idx->emu_block);
			idx->emu_block = malloc(v.block_bytes ? v.block_bytes : 1);
			if (!idx->emu_block) {
				nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
				goto out;
			}
			memcpy(idx->emu_block, blocks, v.block_bytes);
			idx->emu_block_len = v.block_bytes;
			if (pd->want_explain) {
				/*
				 * An emulated rank holds its own block alone: what it can materialise -- and explain,
				 * as a real rank does from its replica -- is its own slice (the other slices' responses
				 * stay NULL, as in own-slice mode).
				 */
				uint8_t *wb = calloc((size_t)W * v.block_bytes + 1, 1);
				int rc;

				if (!wb) {
					nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
					goto out;
				}
				memcpy(wb + (size_t)pd->rank * v.block_bytes, blocks, v.block_bytes);
				rc = resps_from_blocks(nxs, pd, n, W, v.n_slots, v.k, wb, resps, errs, &sb, &failed, pd->rank);
				free(wb);
				if (rc == -1 || (sb.slab && sb.slab->refs && explain_batch(idx, pd, resps, sb.slab) != 0)) {
					goto out;
				}
				if (sb.slab && sb.slab->refs == 0) {
					slab_free(sb.slab);
				}
				ret = failed;
				goto out;
			}
			ret = 0;
			goto out;
		}
		if (resps_from_blocks(nxs, pd, n, W, v.n_slots, v.k, blocks, resps, errs, &sb, &failed,
		    (idx->shard_local && W > 1) ? pd->rank : -1) == -1) {
			goto out;
		}
		idx->hp_resps += now_s() - t0;
	} else {
		/* limit > NXSGPU_BIG_K: the exact two-pass path for the whole batch */
		for (size_t i = 0; i < nl; i++) {
			const qprep_t *q = &pd->prep[i];
			if (!q->errcode && !q->empty) {
				which[nw++] = (uint32_t)i;
			}
		}
		if (run_exact(idx, pd, which, nw, &res, &wres, pos, xtot) != 0) {
			goto out;
		}
		for (size_t j = 0; j < nw; j++) {
			uint32_t at;
			const nxsgpu_results_t *rs = exact_pick(&res, &wres, pos[j], &at);
			total += rs->counts[at];
			if (tot) {
				tot[which[j]] = xtot[j];
			}
		}
		if (slab_begin(&sb, n, total) == -1) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
			goto out;
		}
		for (size_t i = 0, j = 0; i < nl; i++) {
			const qprep_t *q = &pd->prep[i];
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
			{
				uint32_t at;
				const nxsgpu_results_t *rs = exact_pick(&res, &wres, pos[j], &at);
				const uint32_t c = rs->counts[at];

				rp = slab_resp(&sb, i, c);
				memcpy(rp->ids, rs->doc_ids + rs->offsets[at], (size_t)c * 8);
				memcpy(rp->scores, rs->scores + rs->offsets[at], (size_t)c * 4);
				resps[i] = rp;
				j++;
			}
		}
	}
	for (size_t i = 0; tot && i < nl; i++) {
		if (resps[pd->lo + i]) {
			resps[pd->lo + i]->has_total = true;
			resps[pd->lo + i]->total = tot[i];	/* (a query that resolves to nothing: 0) */
		}
	}
	/* (after the exact re-queries have replaced inexact records, before the device index can move) */
	if (pd->want_explain && sb.slab && sb.slab->refs && explain_batch(idx, pd, resps, sb.slab) != 0) {
		goto out;
	}
	if (sb.slab && sb.slab->refs == 0) {
		slab_free(sb.slab);		/* every query failed */
	}
	ret = failed;
out:
	free(tot);
	free(xtot);
	if (ret == -1 && sb.slab) {
		for (size_t i = 0; i < n; i++) {
			resps[i] = NULL;
		}
		slab_free(sb.slab);
	}
	if (res.counts) {
		nxsgpu_results_free(&res);
	}
	if (wres.counts) {
		nxsgpu_results_free(&wres);
	}
	if (patched_own) {
		free(patched);
	}
	free(which);
	free(pos);
	idx->hp_end += now_s() - t_in;
	return ret;
}

int
nxs_index_search_batch(nxs_index_t *idx, nxs_params_t *params,
    const char *const *queries, size_t n, nxs_resp_t **resps, nxs_err_t *errs)
{
	if (pend_oldest(idx)) {
		nxs_clear_error(idx->nxs);
		nxs_decl_err(idx->nxs, NXS_ERR_INVALID,
		    "finish the batches in flight first (nxs_index_search_batch_end)");
		return -1;
	}
	outs_clear(resps, errs, n);
	if (nxs_index_search_batch_begin(idx, params, queries, n) != 0) {
		return -1;
	}
	return nxs_index_search_batch_end(idx, resps, errs);
}

/* ---- similar documents (nxs_index_similar) -------------------------------------------- */

/*
 * The source doc out of a finished response that ran at limit + 1: its entry goes if it is among the results
 * (ids, scores and the explain row move up within the response's own arrays), then the first `limit` stay.
 * The doc matches its own expansions whenever there are any, so a total that counted something counted it.
 */
static void
similar_drop(nxs_resp_t *r, nxs_doc_id_t doc, uint64_t limit)
{
	unsigned at = 0;

	while (at < r->count && r->ids[at] != doc) {
		at++;
	}
	if (at < r->count) {
		const size_t tail = r->count - at - 1;

		memmove(r->ids + at, r->ids + at + 1, tail * sizeof(*r->ids));
		memmove(r->scores + at, r->scores + at + 1, tail * sizeof(*r->scores));
		if (r->n_tok && r->ex_tf && r->ex_imp) {
			/* (the rows live in the slab's explain block, which this response's batch owns) */
			uint32_t *tf = (uint32_t *)(uintptr_t)r->ex_tf;
			float *imp = (float *)(uintptr_t)r->ex_imp;

			memmove(tf + (size_t)at * r->n_tok, tf + (size_t)(at + 1) * r->n_tok, tail * r->n_tok * sizeof(*tf));
			memmove(imp + (size_t)at * r->n_tok, imp + (size_t)(at + 1) * r->n_tok, tail * r->n_tok * sizeof(*imp));
		}
		r->count--;
	}
	if (r->has_total && r->total) {
		r->total--;
	}
	if (r->count > limit) {
		r->count = (unsigned)limit;
	}
	r->iter = 0;
}

int
nxs_index_similar_batch(nxs_index_t *idx, nxs_params_t *params, const nxs_doc_id_t *docs, size_t n,
    nxs_resp_t **resps, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	search_params_t sp;
	uint64_t limit;
	int ret;

	nxs_clear_error(nxs);
	if (pend_oldest(idx)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "finish the batches in flight first (nxs_index_search_batch_end)");
		return -1;
	}
	outs_clear(resps, errs, n);
	if (get_search_params(idx, params, &sp) == -1) {
		return -1;
	}
	/* (a shard's postings are its own: a follow-up, include/nxs.h) */
	if (idx->n_shards) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "similar is not available on a doc shard");
		return -1;
	}
	limit = sp.limit;
	if (!sp.similar_self) {
		if (sp.limit + 1 > UINT_MAX) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid limit");
			return -1;
		}
		sp.limit++;
	}
	/* every term is resolved already */
	sp.fuzzymatch = false;
	sp.prefixmatch = false;
	sp.wildcardmatch = false;
	if (batch_begin(idx, &sp, NULL, docs, n) != 0) {
		return -1;
	}
	ret = nxs_index_search_batch_end(idx, resps, errs);
	for (size_t i = 0; ret >= 0 && !sp.similar_self && i < n; i++) {
		if (resps[i]) {
			similar_drop(resps[i], docs[i], limit);
		}
	}
	return ret;
}

nxs_resp_t *
nxs_index_similar(nxs_index_t *idx, nxs_params_t *params, nxs_doc_id_t doc)
{
	nxs_resp_t *resp = NULL;
	nxsgpu_comm_t *comm = idx->comm;
	int r;

	idx->comm = NULL;	/* one doc is never sharded (as nxs_index_search) */
	r = nxs_index_similar_batch(idx, params, &doc, 1, &resp, NULL);
	idx->comm = comm;
	if (r != 0) {
		if (resp) {
			nxs_resp_release(resp);
		}
		return NULL;
	}
	return resp;
}

#ifdef NXS_TEST_HOOKS
/* the self-removal of nxs_index_similar on a response handed in (built by nxs_test_resp_build) */
void
nxs_test_similar_drop(nxs_resp_t *r, uint64_t doc, uint64_t limit)
{
	similar_drop(r, doc, limit);
}
#endif

/* nxs_index_search: search.c:285-342 (one query = a batch of one) */
nxs_resp_t *
nxs_index_search(nxs_index_t *idx, nxs_params_t *params, const char *query, size_t len)
{
	nxs_resp_t *resp = NULL;
	const char *qv[1] = { query };
	nxsgpu_comm_t *comm = idx->comm;
	int r;

	(void)len;	/* the reference's lexer stops at the NUL byte too (search.c:177) */
	idx->comm = NULL;	/* a single query is never sharded */
	r = nxs_index_search_batch(idx, params, qv, 1, &resp, NULL);
	idx->comm = comm;
	if (r != 0) {
		if (resp) {
			nxs_resp_release(resp);
		}
		return NULL;
	}
	return resp;
}

/* ---- query sharding over the GPUs of a node ---------------------------------------- */

int
nxs_shard_unique_id(nxs_t *nxs, uint8_t *uid)
{
	nxs_clear_error(nxs);
	if (nxsgpu_comm_unique_id(uid) != 0) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "%s", nxsgpu_last_error());
		return -1;
	}
	return 0;
}

int
nxs_index_shard(nxs_index_t *idx, int rank, int world, const uint8_t *uid)
{
	nxs_t *nxs = idx->nxs;

	nxs_clear_error(nxs);
	if (pend_oldest(idx)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "batches are in flight");
		return -1;
	}
	if (idx->comm) {
		(void)nxsgpu_index_set_comm(idx->dev, NULL);
		nxsgpu_comm_destroy(idx->comm);
		idx->comm = NULL;
	}
	if (world <= 1 && !uid) {
		return 0;	/* detach */
	}
	idx->comm = nxsgpu_comm_create(idx->device, rank, world, uid);
	if (!idx->comm || nxsgpu_index_set_comm(idx->dev, idx->comm) != 0) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "sharding setup failed: %s", nxsgpu_last_error());
		nxsgpu_comm_destroy(idx->comm);
		idx->comm = NULL;
		return -1;
	}
	return 0;
}

/*
 * The reference scales out by independent worker processes, each answering only ITS OWN requests
 * (compose/nginx.conf:2).  nxs_index_shard_local(idx, true): a rank of a sharded index materialises the
 * responses of its own slice only -- resps[i] stays NULL and errs[i] is left alone for the queries the other
 * ranks own; the return value counts the failures of the own slice.  The collective is unchanged (every rank
 * still sees every block: aborts, the fix-up round and re-sync agreement read all status words), but the
 * per-rank host work per batch is O(n / world) instead of O(n).
 */
int
nxs_index_shard_local(nxs_index_t *idx, bool on)
{
	nxs_clear_error(idx->nxs);
	if (pend_oldest(idx)) {
		nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "batches are in flight");
		return -1;
	}
	idx->shard_local = on;
	return 0;
}

/* the part [*lo, *hi) of an n-query batch whose responses this index delivers (everything unless
 * nxs_index_shard_local is on and a communicator of more than one rank -- or its emulation -- is attached) */
void
nxs_index_shard_slice(const nxs_index_t *idx, size_t n, size_t *lo, size_t *hi)
{
	const int world = idx->comm ? nxsgpu_comm_world(idx->comm) : idx->emu_world;
	const int rank = idx->comm ? nxsgpu_comm_rank(idx->comm) : idx->emu_rank;
	uint64_t a = 0, b = n;

	if (idx->shard_local && world > 1) {
		nxsgpu_shard_slice(n, rank, world, &a, &b);
	}
	*lo = (size_t)a;
	*hi = (size_t)b;
}

#ifdef NXS_TEST_HOOKS
/*
 * Sharding without a second GPU.  nxs_test_shard_emulate(idx, r, W) makes the
 * index play rank r of a W-rank run with the collective left out: the next
 * batch plans and runs rank r's slice, and nxs_test_shard_block() hands out
 * the record block it would have contributed to the all-gather (W = 0: off).
 * nxs_test_pack_record() writes one record + status word into a block (a
 * CPU-side stand-in for the device in the gloo test), and
 * nxs_test_assemble() is the reassembly every rank runs on the gathered blocks.
 */
void
nxs_test_shard_emulate(nxs_index_t *idx, int rank, int world)
{
	idx->emu_rank = rank;
	idx->emu_world = world;
}

size_t
nxs_test_shard_block(nxs_index_t *idx, uint8_t *out, size_t cap)
{
	if (out && idx->emu_block && idx->emu_block_len <= cap) {
		memcpy(out, idx->emu_block, idx->emu_block_len);
	}
	return idx->emu_block ? idx->emu_block_len : 0;
}

void
nxs_test_pack_record(uint8_t *block, uint32_t n_slots, uint32_t k, uint32_t slot,
    uint32_t count, const uint64_t *ids, const float *scores, uint32_t status)
{
	uint8_t *rec = block + (size_t)slot * NXSGPU_REC_BYTES(k);
	uint32_t *st = (uint32_t *)(block + (size_t)n_slots * NXSGPU_REC_BYTES(k));

	((uint32_t *)rec)[0] = count;
	((uint32_t *)rec)[1] = 0;
	memcpy(rec + 8, ids, (size_t)count * 8);
	memcpy(rec + 8 + 8 * (size_t)k, scores, (size_t)count * 4);
	st[slot] = status;
}

/* mark a record "inexact" (candidate overflow: the owner re-runs the query in the fix-up round) */
void
nxs_test_mark_inexact(uint8_t *block, uint32_t n_slots, uint32_t k, uint32_t slot)
{
	(void)n_slots;
	((uint32_t *)(block + (size_t)slot * NXSGPU_REC_BYTES(k)))[1] = NXSGPU_REC_INEXACT;
}

/* the block's flags word says "this rank saw the index files move" ... */
void
nxs_test_mark_changed(uint8_t *block, uint32_t n_slots, uint32_t k)
{
	((uint32_t *)(block + (size_t)n_slots * NXSGPU_REC_BYTES(k)))[n_slots] |= NXSGPU_BLOCK_CHANGED;
}

/* ... and what every rank reads off the gathered blocks: re-sync at the next _begin? */
int
nxs_test_blocks_changed(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k)
{
	return blocks_changed(blocks, world, n_slots, k) ? 1 : 0;
}

/* what every rank reads off the gathered blocks: does the batch need a fix-up round, and which
 * of `rank`'s own queries (local indexes) have to be re-run?  -> 1 / 0, *nw set */
int
nxs_test_fixup_scan(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k, size_t n,
    int rank, uint32_t *which, size_t *nw)
{
	*nw = 0;
	return fixup_scan(blocks, true, world, rank, n_slots, k, n, which, nw) ? 1 : 0;
}

/* ... and off the blocks of the second all-gather: -1 = fine, else the rank that failed the batch */
int
nxs_test_fixup_verify(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k, size_t n)
{
	nxs_err_t acode = NXS_ERR_SUCCESS;
	return fixup_verify(blocks, world, n_slots, k, n, &acode);
}

/* what a rank that cannot do its share contributes instead (STATUS_ABORT) */
void
nxs_test_pack_abort(uint8_t *block, uint32_t n_slots, uint32_t k, uint32_t code)
{
	uint32_t *st = (uint32_t *)(block + (size_t)n_slots * NXSGPU_REC_BYTES(k));

	memset(block, 0, NXSGPU_BLOCK_BYTES(n_slots, k));
	for (uint32_t i = 0; i < n_slots; i++) {
		st[i] = STATUS_ABORT | code;
	}
}

/* the n-th next _begin (which = 0) / exact fix-up round (1) of the index fails; 2: the n-th next
 * fix-up round finds no memory for its receive buffer; 3: the n-th next late second half (late_complete) fails;
 * 4: the n-th next device step (merge or rebuild) of a doc-shard refresh fails */
void
nxs_test_inject_failure(nxs_index_t *idx, int which, unsigned nth)
{
	if (which == 4) {
		idx->test_fail_dsref = nth;
	} else if (which == 0) {
		idx->test_fail_begin = nth;
	} else if (which == 1) {
		idx->test_fail_fixup = nth;
	} else if (which == 3) {
		idx->test_fail_late = nth;
	} else {
		idx->test_fail_fixup_recv = nth;
	}
}

/* >= 0: failed queries; -1: error; <= -2: rank (-2 - ret) aborted the batch --
 * every rank sees that and fails the batch, none is left in a collective */
int
nxs_test_assemble(const uint8_t *blocks, uint32_t world, uint32_t n_slots, uint32_t k,
    size_t n, nxs_resp_t **resps, nxs_err_t *errs, int only_rank)
{
	nxs_t fake;
	slab_builder_t sb = { 0 };
	int failed = 0, ar;
	nxs_err_t acode;

	memset(&fake, 0, sizeof(fake));
	outs_clear(resps, errs, n);
	if ((ar = blocks_aborted(blocks, world, n_slots, k, &acode)) >= 0) {
		for (size_t i = 0; i < n; i++) {
			errs[i] = acode;
		}
		return -2 - ar;
	}
	if (resps_from_blocks(&fake, NULL, n, world, n_slots, k, blocks, resps, errs, &sb, &failed, only_rank) == -1) {
		free(fake.errmsg);
		return -1;
	}
	if (sb.slab && sb.slab->refs == 0) {
		slab_free(sb.slab);
	}
	free(fake.errmsg);
	return failed;
}

/*
 * Where the host's time goes, summed over the batches so far: out[0] parse +
 * resolve + compile (worker pool), out[1] queueing the batch on the device
 * (work list, staging, launches), out[2] waiting for the device, out[3]
 * building the responses; out[4] = batches; out[8] = the part of out[0] spent waiting for the device's
 * fuzzy pass.  Reset on read.
 */
void
nxs_index_host_profile(nxs_index_t *idx, double out[12])
{
	out[8] = idx->hp_fzwait;	/* of out[0]: waiting for the device's fuzzy pass, */
	out[9] = idx->hp_front;		/* parse + lookups (+ compile of the queries without misses), */
	out[10] = idx->hp_fzlaunch;	/* queueing the fuzzy pass, */
	out[11] = idx->hp_back;		/* winners into the plans + compile of the rest */
	idx->hp_fzwait = idx->hp_front = idx->hp_fzlaunch = idx->hp_back = 0;
	out[6] = idx->hp_begin;		/* whole _begin() / _end() calls */
	out[7] = idx->hp_end;
	idx->hp_begin = idx->hp_end = 0;
	out[5] = (double)idx->hp_inexact;	/* queries re-run on the exact path */
	idx->hp_inexact = 0;
	out[0] = idx->hp_plan;
	out[1] = idx->hp_queue;
	out[2] = idx->hp_wait;
	out[3] = idx->hp_resps;
	out[4] = (double)idx->hp_batches;
	idx->hp_plan = idx->hp_queue = idx->hp_wait = idx->hp_resps = 0;
	idx->hp_batches = 0;
}

void
nxs_index_shard_info(nxs_index_t *idx, uint64_t out[4])
{
	uint64_t st[2] = { 0, 0 };

	out[0] = (uint64_t)(int64_t)(idx->comm ? nxsgpu_comm_rccl_count(idx->comm) : -1);
	out[1] = idx->comm ? (uint64_t)nxsgpu_comm_world(idx->comm) : 1;
	nxsgpu_comm_stats(idx->comm, st);
	out[2] = st[0];
	out[3] = st[1];
}
#endif /* NXS_TEST_HOOKS */
