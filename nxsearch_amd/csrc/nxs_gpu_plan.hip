/*
 * nxs_gpu_plan.hip -- host only: which kernel class a query gets, the work list of a batch, and where
 * the batch's arrays live (MI355X / gfx950 query path of nxsearch; see nxs_gpu_int.h for the map of the files)
 */
#include "nxs_gpu_int.h"

/*
 * Work decomposition: every query's doc space is cut into n_groups equal
 * ranges (multiples of TILE_W), one wavefront each.  The number of ranges is
 * proportional to the query's share of the batch's postings, so a query with
 * long lists gets many wavefronts and a sparse one a single one (whose fixed
 * costs -- cursor searches, warm-up of the candidate threshold -- are then
 * paid once).  Items are grouped by kernel class (token-count bucket x
 * tile/step path) and emitted heaviest query first inside a class.
 *
 * build_worklist: classify_query per query, merge_stragglers, size_ranges, emit_launches.
 */

void
delete_worklist(worklist_t *wl)
{
	delete wl;
}

static uint32_t
nt_bucket(uint32_t nt)
{
	return nt <= 1 ? 1 : nt <= 2 ? 2 : nt <= 3 ? 3 : nt <= 5 ? 5 : 8;
}

/* what the steps share: the index, its switches and what the batch is */
struct plan_ctx_t {
	const nxsgpu_index_t *ix;
	const gpu_cfg_t &cf;
	bool		solo;		/* a small batch that has the GPU to itself */
	uint32_t	big_k;		/* the limit if > 64, else 0 */
	/* (limits > 64 -- big_k -- filter on a histogram threshold: the accumulator tiles,
	 * k_scanr and k_scan1 have that mode, the mask path and the dense-term class do not) */
	bool		use_scanr, use_scanm;

	plan_ctx_t(const nxsgpu_index_t *ix_, bool solo_, uint32_t big_k_) : ix(ix_), cf(ix_->cfg), solo(solo_), big_k(big_k_),
	    use_scanr(cf.use_scanr && ix_->n_docs < (1ull << 31)),
	    use_scanm(cf.use_scanm && ix_->n_docs < (1ull << 31) && big_k_ == 0) {}
	/* the stripes' slices of the lists are table lookups: every term needs a rank directory */
	bool have_stripes() const { return cf.use_scans && ix->n_post < (1ull << 32) && ix->d_bmrank; }
};

static uint64_t
list_len(const dev_query_t &q, uint32_t t)
{
	return q.pend[t] - q.pbeg[t];
}

/* a query's work changes: the batch's total follows */
static void
set_work(uint64_t &work, uint64_t &total, uint64_t w)
{
	total -= work;
	work = w;
	total += work;
}

/* every token outside `except` has a block-presence bitmap / rank directory */
static bool
all_have_bitmaps(const dev_query_t &q, uint32_t except = 0)
{
	bool all = true;
	for (uint32_t t = 0; t < q.nt; t++) {
		all = all && (((except >> t) & 1) || q.bm_col[t] != 0xffffffffu);
	}
	return all;
}

/*
 * Step 1: the class of one query and its work in postings (added to `total`).  A TF-IDF query that takes
 * the sparse + dense class has the lists of its dropped tokens replaced by their outlier lists in `q`.
 */
static qclass_t
classify_query(const plan_ctx_t &P, dev_query_t &q, uint64_t &work, uint64_t &total)
{
	const nxsgpu_index_t *ix = P.ix;
	const gpu_cfg_t &cf = P.cf;
	const uint32_t bucket = nt_bucket(q.nt);
	uint64_t w = 0, wmax = 0;

	for (uint32_t t = 0; t < q.nt; t++) {
		w += list_len(q, t);
		wmax = std::max(wmax, list_len(q, t));
	}
	work = w;
	total += w;
	if (q.nt > 8) {
		return qclass_t{ CLS_GENERIC, SHAPE_MASK, 0 };
	}
	/* pure OR: every non-empty presence mask matches => no mask array */
	bool or_only = q.nt >= 2 && cf.mask_off;
	for (uint32_t m = 1; or_only && m < (1u << q.nt); m++) {
		or_only = (q.truth[m >> 5] >> (m & 31)) & 1;
	}
	const uint32_t shape = or_only ? SHAPE_OR : SHAPE_MASK;
	qclass_t c = { CLS_TILES, shape, bucket };
	/* pure OR of 2..8 tokens whose lists are sparse: mask path (k_scanm).
	 * Dense lists stream faster through the accumulator tiles. */
	/* ... or any expression without a required token: the bound in the
	 * byte map does not depend on the operators, the truth table is
	 * applied to the few docs that get scored
	 * (only where matches are common enough for a threshold to form:
	 * at least half of the tokens satisfy the expression on their own --
	 * "(a AND b) OR (c AND d)" floods the scoring stage and stays on the
	 * accumulator tiles: 3.3 ms there, 5.4 ms here) */
	uint32_t singles = 0;
	for (uint32_t t = 0; t < q.nt && t < 8; t++) {
		const uint32_t m1 = 1u << t;
		singles += (q.truth[m1 >> 5] >> (m1 & 31)) & 1;
	}
	const bool no_req = q.req == 0 && q.nt >= 2 && q.nt <= 8 && 2 * singles >= q.nt;
	const bool nt_ok = q.nt >= cf.scanm_minnt && q.nt <= cf.scanm_maxnt;
	/* (k_scanm if the densest list holds at most scanm_dens of the docs) */
	if ((or_only || (no_req && cf.scanm_general)) && P.use_scanm && nt_ok &&
	    (double)wmax <= cf.scanm_dens * (double)ix->n_docs) {
		c.kind = CLS_SCANM;
		/* ... on presence bits (k_scanb) where that kernel is the faster one: its cost per
		 * posting does not fall with the lists' density as the byte map's does, so it
		 * takes the queries whose lists TOGETHER hold few docs (measured cross-over on
		 * 10M docs: 5-term ORs of rank 500-1000 -29 %, of rank 100-1000 +9 %) */
		if (cf.use_scanb && q.nt <= 5 && (double)w <= cf.scanb_dens * (double)ix->n_docs) {
			c.kind = CLS_SCANB;
		}
		/* ... on doc stripes (k_scans) when every term has a rank directory: the stripes'
		 * slices of the lists are table lookups, no per-term window state */
		if (c.kind == CLS_SCANM && P.have_stripes() && all_have_bitmaps(q)) {
			c.kind = CLS_SCANS;
			/* (longer ranges: a stripe range's fixed costs -- set-up, the cold sub-ranges, ~1.3 flushes --
			 * are paid per wavefront) */
			if (cf.scans_workpct != 100) {
				set_work(work, total, std::max<uint64_t>(1, work * cf.scans_workpct / 100));
			}
		}
	} else if (or_only && P.use_scanm && cf.use_drop && q.drop_mask && nt_ok) {
		/*
		 * A pure OR of sparse terms AND dense ones: the mask path on the
		 * sparse terms, the dense lists leave the scan once the threshold
		 * exceeds their joint ceiling (k_scanm<.., DROP>).  Needs enough
		 * sparse postings for a threshold to form in every doc range; the
		 * work is what the sparse lists hold.
		 */
		uint64_t ws = 0;
		uint32_t n_sparse = 0;
		for (uint32_t t = 0; t < q.nt; t++) {
			if (!((q.drop_mask >> t) & 1)) {
				ws += list_len(q, t);
				n_sparse++;
			} else if (q.outl_tfidf) {
				const size_t col = q.drop_col[t];
				ws += ix->outl_off[col + 1] - ix->outl_off[col];	/* (a dropped term's outlier list is scanned) */
			}
		}
		if (n_sparse && ws >= cf.drop_minpost) {
			/* TF-IDF: from here on the dropped tokens' lists are their outlier lists
			 * (kernels that stream the terms' own lists must not see this query again:
			 * qflags) */
			for (uint32_t t = 0; t < q.nt && q.outl_tfidf && !cf.drop_tiles; t++) {
				const size_t col = q.drop_col[t];
				if (((q.drop_mask >> t) & 1) && ix->outl_off[col + 1] > ix->outl_off[col]) {
					q.pbeg[t] = ix->outl_off[col];
					q.pend[t] = ix->outl_off[col + 1];
					q.outl_mask |= 1u << t;
					q.qflags |= 1;
				}
			}
			if (!cf.drop_tiles) {
				set_work(work, total, cf.drop_workmul * (ws + 16384));	/* latency-bound wavefronts: more, shorter ranges */
			}
			c = qclass_t{ CLS_DROP_M, SHAPE_OR, bucket };
			/* ... on doc stripes (k_cold + k_scans<.., DROP>) if the sparse terms all have a rank
			 * directory and no dropped term brings an outlier list (those have none) */
			if (cf.use_scans_drop && !q.outl_tfidf && ix->d_dense_q8 && P.have_stripes() && !q.outl_mask &&
			    all_have_bitmaps(q, q.drop_mask)) {
				c.kind = CLS_DROP_S;
			}
		}
	}
	/* required terms: intersect first (k_scanr).  Its work is set by
	 * the shortest required list; longer lists are mostly skipped */
	if (q.n_req && q.nt >= P.cf.rmin /* 3: "a AND b" takes k_scan8's sign-bit path */ && P.use_scanr) {
		const uint64_t dfd = list_len(q, q.slot_tok[0]);
		uint64_t wr = 0;
		for (uint32_t t = 0; t < q.nt; t++) {
			wr += std::min<uint64_t>(list_len(q, t), 4 * dfd);
		}
		set_work(work, total, wr);
		/* (four required terms and more: rounds of whole driver windows, k_scanr<.., true>) */
		c = qclass_t{ CLS_SCANR, (SCANR_HASH && q.n_req >= 4) ? SHAPE_OR : SHAPE_MASK, bucket };
		/*
		 * Two required terms and more that all have a block-presence bitmap: AND the
		 * bitmaps and look at the postings of the surviving 64-doc blocks only
		 * (k_scanq) -- if few blocks are expected to survive (independent lists: a
		 * block holds term t with probability 1 - (1 - df_t / N)^64) against what
		 * the driver list would cost k_scanr.
		 */
		if (cf.use_blkmap && q.n_req >= 2 && ix->n_post < (1ull << 32)) {
			double surv = (double)ix->n_docs / 64.0;
			double em = (double)ix->n_docs;		/* expected docs holding every required term */
			for (uint32_t t = 0; t < q.nt; t++) {
				if (!((q.req >> t) & 1)) {
					continue;
				}
				const double rho = (double)list_len(q, t) / (double)std::max<uint64_t>(ix->n_docs, 1);
				double e64 = 1.0 - std::min(rho, 1.0);	/* ^64 by squaring (std::pow: 2 500 calls a batch) */
				e64 *= e64; e64 *= e64; e64 *= e64; e64 *= e64; e64 *= e64; e64 *= e64;
				surv *= 1.0 - e64;
				em *= std::min(rho, 1.0);
			}
			/* (limits > 64: k_scanq<.., BIG> emits EVERY match -- for queries that expect a
			 * handful; more than a range's candidate list holds sends the query to the exact path) */
			if (all_have_bitmaps(q, ~q.req) && surv * cf.bm_gain < (double)dfd && (P.big_k == 0 || em < cf.bigq_em)) {
				/* the bitmaps' words + the surviving blocks (a lane each), in posting units */
				set_work(work, total, (uint64_t)(ix->n_docs / 256 + surv * 64.0) + 1);
				c.kind = CLS_SCANQ;
			}
		}
	}
	return c;
}

/*
 * Step 2: stragglers.  A pure-OR query whose lists are too dense for the mask path and that
 * cannot drop them either (two dense terms, a ceiling too close to the sparse ones)
 * takes the accumulator tiles -- a class of ONE or two queries in a C3 batch: a launch
 * of its own on the scan stream, 0.1 ms of latency for 8 MB of postings, with nothing
 * to run beside.  The mask kernel takes any density (it is merely slower per dense
 * posting): up to four such queries join the batch's mask-path class of their shape,
 * where their ranges are wavefronts among tens of thousands.
 * (NXS_GPU_NOSTRAGGLER: such classes stay launches of their own.)
 */
static void
merge_stragglers(const plan_ctx_t &P, const dev_query_t *hq, uint32_t nq, std::vector<qclass_t> &cls)
{
	const gpu_cfg_t &cf = P.cf;
	uint32_t n_in[CLS_SLOTS] = { 0 };

	if (cf.no_straggler || !P.use_scanm) {
		return;
	}
	for (uint32_t i = 0; i < nq; i++) {
		n_in[cls[i].slot()]++;
	}
	/* (the batch's mask-path class of a shape: on doc stripes -- k_scans -- if the query's terms all have
	 * a rank directory and that class is the populated one, else on register windows) */
	auto mask_class = [&](uint32_t i, uint32_t shape, uint32_t bucket) -> qclass_t {
		const qclass_t stripes = { CLS_SCANS, shape, bucket }, windows = { CLS_SCANM, shape, bucket };
		return (P.have_stripes() && all_have_bitmaps(hq[i]) && n_in[stripes.slot()] >= 32) ? stripes : windows;
	};
	for (uint32_t i = 0; i < nq; i++) {
		const qclass_t c = cls[i];
		if (c.kind == CLS_TILES && c.shape == SHAPE_OR && c.bucket >= 2 && n_in[c.slot()] <= 4 &&
		    hq[i].nt >= cf.scanm_minnt && hq[i].nt <= cf.scanm_maxnt) {
			const qclass_t to = mask_class(i, SHAPE_OR, c.bucket);
			if (n_in[to.slot()] >= 32) {
				cls[i] = to;
			}
		}
		/* (the same for a handful of very sparse queries that would take k_scanb: a launch of
		 * their own only pays with enough of them) */
		if (c.kind == CLS_SCANB && n_in[c.slot()] < 64) {
			const qclass_t to = mask_class(i, c.shape, c.bucket);
			if (n_in[to.slot()] >= 32) {
				cls[i] = to;
			}
		}
	}
}

/*
 * Step 3: every query's ranges -- how many, how many docs each, their segments -- from its work and the
 * batch's total; fills wl.qmeta, wl.n_segs, wl.need_cursors and wl.bnd_q.
 */
static void
size_ranges(const plan_ctx_t &P, const std::vector<qclass_t> &cls, const std::vector<uint64_t> &work, uint64_t total,
    uint32_t nq, worklist_t &wl)
{
	const nxsgpu_index_t *ix = P.ix;
	const gpu_cfg_t &cf = P.cf;
	const uint64_t tiles = std::max<uint64_t>(1, (ix->n_docs + TILE_W - 1) / TILE_W);
	/* (a batch that has the GPU to itself is latency-bound: shorter ranges, more of them) */
	const uint64_t min_post = P.solo ? std::min(cf.min_post, cf.min_post_solo) : cf.min_post;

	/* (limits > 64: a range's own threshold needs well over k matches to form, and
	 * every range that starts cold emits k candidates before it has one) */
	/* (a batch with the stripe class: somewhat longer ranges for everything -- measured on C3, 57 344 against 65 536
	 * wavefronts with the class itself at 70 %: 1.00 -> 1.05 M queries/s; single-token batches keep the finer split) */
	bool any_scans = false;
	for (uint32_t i = 0; i < nq && !any_scans; i++) {
		any_scans = cls[i].kind == CLS_SCANS;
	}
	/* (... and a huge batch -- C5: 29 G postings -- more wavefronts than the target: a range of more than cf.max_post
	 * postings leaves the step's tail to a few long wavefronts (C5: 358k -> 377k queries/s); at most four times the target: the staging area's bound) */
	uint64_t target_eff = any_scans ? cf.wave_target_scans : cf.wave_target;
	target_eff = std::min<uint64_t>(4 * target_eff, std::max<uint64_t>(target_eff, total / std::max<uint64_t>(cf.max_post, 1)));
	const uint64_t per_wave = std::max<uint64_t>(std::max<uint64_t>(min_post, (uint64_t)P.big_k * cf.big_minpost),
	    total / std::max<uint64_t>(target_eff, 1) + 1);

	wl.qmeta.assign(nq, qmeta_t());
	wl.n_segs = 0;
	wl.need_cursors = false;
	for (uint32_t i = 0; i < nq; i++) {
		uint64_t per_i = per_wave;
		if (P.solo) {
			/*
			 * Alone on the GPU every range starts cold and emits its own early
			 * maxima (~10 (1 + ln(postings / 10)) candidates each), which the replay
			 * then streams through one wavefront; a range's scan is a chain of
			 * dependent window loads.  Scan time falls with the number of ranges R,
			 * replay time grows with it: the sum is smallest near R = sqrt(n / 84),
			 * i.e. sqrt(84 n) postings per range (2M postings: 154 ranges, not 2000).
			 */
			/* (never finer than the batch-wide rule: the work list's size bound rests on it) */
			per_i = std::max<uint64_t>(per_wave, (uint64_t)std::sqrt(84.0 * (double)work[i]));
		}
		uint64_t g = std::max<uint64_t>(1, (work[i] + per_i - 1) / per_i);
		g = std::min<uint64_t>(g, tiles);
		g = std::min<uint64_t>(g, 65535);
		const uint64_t tiles_per = (tiles + g - 1) / g;
		g = (tiles + tiles_per - 1) / tiles_per;
		qmeta_t &m = wl.qmeta[i];
		m.n_groups = (uint32_t)g;
		m.group_docs = (uint32_t)std::min<uint64_t>(tiles_per * TILE_W, 0xffffffffu & ~(uint64_t)(TILE_W - 1));
		/* single-token queries on k_scan1: any split of the list into contiguous
		 * pieces, highest docs first, feeds the heap the same sequence -- split by
		 * posting index and the batch needs no k_cursors launch */
		m.pad = (cls[i].kind == CLS_TILES && cls[i].bucket == 1 && !cf.no_scan1 && !cf.old_scan &&
		    ix->n_docs < (1ull << 31)) ? 1u : 0u;
		wl.need_cursors = wl.need_cursors || m.pad == 0;
	}
	for (uint32_t i = 0; i < nq; i++) {
		wl.qmeta[i].seg_first = wl.n_segs;
		wl.n_segs += wl.qmeta[i].n_groups;
	}
	/* (both arrays are sized once and written through plain pointers: 130 000 push_back calls cost 0.1 ms a batch) */
	wl.bnd_q.resize((size_t)wl.n_segs + nq);
	uint32_t *bp = wl.bnd_q.data();
	for (uint32_t i = 0; i < nq; i++) {
		/* query i owns boundaries seg_first + i ... + n_groups (inclusive) */
		bp = std::fill_n(bp, (size_t)wl.qmeta[i].n_groups + 1, i);
	}
}

/* launch order of the classes: the mask path first -- a class's heap replay
 * runs beside the NEXT class's scan, and the last class (required-term
 * queries: few candidates, short replay) is the one left exposed */
/* (the sparse + dense class leads: it runs on a stream of its own, beside the rest) */
static uint32_t
launch_rank(uint32_t kind)
{
	static const uint32_t rank[CLS_KINDS] = {
		/* GENERIC */ 5, /* TILES */ 6, /* (2) */ 0, /* SCANR */ 7, /* SCANM */ 3, /* DROP_M */ 1,
		/* SCANB */ 4, /* SCANQ */ 8, /* SCANS */ 2, /* DROP_S */ 0
	};
	return rank[kind];
}

/* the class's items so far leave in a launch of their own, ahead of the rest (no query ends in it) */
static void
send_ahead(worklist_t &wl, launch_t &l, uint32_t o0, size_t n_items)
{
	launch_t l0 = l;
	l0.count = (uint32_t)n_items - l0.first;
	l0.q_first = o0;
	l0.q_count = 0;			/* (no replay behind this one) */
	l0.postings = 0;		/* (the class's postings are charged to the launch its queries end in) */
	wl.launches.push_back(l0);
	l.first = (uint32_t)n_items;
}

/*
 * Step 4: the queries in launch order (wl.qorder), their items and one launch per class (wl.items,
 * wl.launches), heaviest query first inside a class.
 */
static void
emit_launches(const plan_ctx_t &P, const dev_query_t *hq, const std::vector<qclass_t> &cls,
    const std::vector<uint64_t> &work, uint32_t nq, worklist_t &wl)
{
	const gpu_cfg_t &cf = P.cf;
	std::vector<uint32_t> &order = wl.qorder;

	order.resize(nq);
	for (uint32_t i = 0; i < nq; i++) {
		order[i] = i;
	}
	std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
		const qclass_t &cx = cls[x], &cy = cls[y];
		if (cx.kind != cy.kind) return launch_rank(cx.kind) < launch_rank(cy.kind);
		if (cx.shape != cy.shape) return cx.shape < cy.shape;
		if (cx.bucket != cy.bucket) return cx.bucket < cy.bucket;
		return work[x] != work[y] ? work[x] > work[y] : x < y;
	});
	wl.launches.clear();
	wl.items.resize(wl.n_segs);
	item_t *const items = wl.items.data();
	size_t n_items = 0;
	/*
	 * Inside a class, items go out level by level: level l of every query
	 * (its l-th highest doc range) before level l+1 of any.  All items carry
	 * about per_wave postings, so this costs no balance, and it spreads one
	 * query's ranges in time: when a range starts, higher ranges of its query
	 * have usually finished and published their threshold (range_hint).
	 */
	for (uint32_t o0 = 0; o0 < nq; ) {
		const qclass_t c = cls[order[o0]];
		uint32_t o1 = o0, max_g = 0;
		while (o1 < nq && cls[order[o1]] == c) {
			max_g = std::max(max_g, wl.qmeta[order[o1]].n_groups);
			o1++;
		}
		launch_t l;
		l.postings = 0;
		l.first = (uint32_t)n_items;
		l.nt_bucket = c.bucket;
		l.nomask = c.shape;
		l.kind = c.kind;
		if (cf.by_level) {
			/* the class is sorted by work, so n_groups does not increase along
			 * it (checked): the queries that still have a level `lev` form a
			 * prefix, and the loop is linear in the number of items */
			bool mono = true;
			for (uint32_t oi = o0 + 1; oi < o1 && mono; oi++) {
				mono = wl.qmeta[order[oi]].n_groups <= wl.qmeta[order[oi - 1]].n_groups;
			}
			uint32_t live_end = o1;
			for (uint32_t lev = 0; lev < max_g; lev++) {
				while (mono && live_end > o0 && wl.qmeta[order[live_end - 1]].n_groups <= lev) {
					live_end--;
				}
				for (uint32_t oi = o0; oi < live_end; oi++) {
					const uint32_t i = order[oi];
					if (lev < wl.qmeta[i].n_groups) {
						item_t it;
						it.q = i;
						it.g = wl.qmeta[i].n_groups - 1 - lev;
						items[n_items++] = it;
					}
				}
				if (P.big_k || P.solo) {
					continue;
				}
				/*
				 * The sparse + dense class (k_cold + k_scanm<.., DROP>) of a mixed batch is a few
				 * thousand wavefronts: ALL of them fit the GPU at once, so no range ever finds a
				 * threshold published by a higher one -- every range walks its cold phase and
				 * pushes on a weak threshold (8 x the pending docs of the plain class).  The first
				 * level(s) go ahead in a launch of their own.
				 */
				if (lev + 1 == cf.drop_split && cls_sparse_dense(c.kind) && max_g > cf.drop_split) {
					send_ahead(wl, l, o0, n_items);
				}
				/*
				 * Single-token queries (k_scan1: a wavefront is ~20 us of streaming):
				 * a dense term is thousands of ranges that would all start at once,
				 * cold, each handing its ~10 (1 + ln(postings / 10)) early maxima to
				 * the one wavefront that replays the query -- 150 000 candidates for a
				 * term holding 90 % of 10M docs, 0.3 ms of replay behind 0.05 ms of
				 * scanning.  The TOP range of every query goes first, in a launch of
				 * its own: when the others start it has published the 10th best of its
				 * 4096 postings, and they emit a seventh of that.
				 */
				if (lev == 0 && c.kind == CLS_TILES && c.bucket == 1 && max_g >= cf.scan1_split) {
					send_ahead(wl, l, o0, n_items);
				}
			}
		} else {
			for (uint32_t oi = o0; oi < o1; oi++) {
				const uint32_t i = order[oi];
				for (uint32_t g = wl.qmeta[i].n_groups; g-- > 0; ) {
					item_t it;
					it.q = i;
					it.g = g;
					items[n_items++] = it;
				}
			}
		}
		l.count = (uint32_t)n_items - l.first;
		l.q_first = o0;
		l.q_count = o1 - o0;
		l.postings = 0;
		for (uint32_t oi = o0; oi < o1; oi++) {
			const dev_query_t &dq = hq[order[oi]];
			for (uint32_t t = 0; t < dq.nt; t++) {
				/* (a dropped token whose list was replaced by its outlier list: the term's own df is not known
				 * here any more -- the class's figure then counts what is scanned) */
				l.postings += list_len(dq, t);
			}
		}
		wl.launches.push_back(l);
		o0 = o1;
	}
}

void
build_worklist(const nxsgpu_index_t *ix, dev_query_t *hq, uint32_t nq, worklist_t &wl, bool solo, uint32_t big_k)
{
	const plan_ctx_t P(ix, solo, big_k);
	std::vector<uint64_t> work(nq);
	std::vector<qclass_t> cls(nq);
	uint64_t total = 0;

	for (uint32_t i = 0; i < nq; i++) {
		cls[i] = classify_query(P, hq[i], work[i], total);
	}
	merge_stragglers(P, hq, nq, cls);
	size_ranges(P, cls, work, total, nq, wl);
	emit_launches(P, hq, cls, work, nq, wl);
}

/* ---- where a batch's arrays live ------------------------------------------------------------------ */

batch_layout_t
batch_layout(uint8_t *base, const batch_dims_t &d)
{
	batch_layout_t L;
	uint8_t *p = base;
	const size_t nq = d.nq, nseg = d.nseg;

	L.q = carve<dev_query_t>(p, nq);
	L.qmeta = carve<qmeta_t>(p, nq);
	L.items = carve<item_t>(p, nseg);
	L.bnd_q = carve<uint32_t>(p, nseg + nq);
	L.qorder = carve<uint32_t>(p, nq);
	L.rec_slot = carve<uint32_t>(p, d.rec_slots ? nq : 0);
	L.pub = carve<float>(p, nseg);
	L.retry_cnt = carve<uint32_t>(p, RETRY_LISTS);
	L.ovf = carve<uint32_t>(p, nq);
	L.totals = d.totals ? carve<uint32_t>(p, nq) : NULL;	/* (absent: not even the alignment) */
	L.up_len = (size_t)(p - base);
	L.out_ids = carve<uint64_t>(p, d.results ? nq * d.k : 0);
	L.out_sc = carve<float>(p, d.results ? nq * d.k : 0);
	L.out_cnt = carve<uint32_t>(p, d.results ? nq : 0);
	L.down_len = (size_t)(p - (uint8_t *)L.ovf);
	L.status = carve<uint32_t>(p, d.status_words);
	L.host_len = (size_t)(p - base);
	L.seg_count = carve<uint32_t>(p, nseg);
	L.cursors = carve<uint32_t>(p, (nseg + nq) * NXSGPU_MAX_TOKENS);
	L.cand_doc = carve<uint32_t>(p, nseg * d.seg_cap);
	L.cand_sc = carve<float>(p, nseg * d.seg_cap);
	L.cold_state = carve<uint32_t>(p, nseg * 16);
	L.cold_top = carve<float>(p, nseg * 64);
	L.retry_items = carve<item_t>(p, RETRY_LISTS * RETRY_CAP);
	L.pub_sk = carve<float>(p, d.big ? nseg * 8 : 0);
	L.log_ids = carve<uint64_t>(p, d.log_cap ? nq * d.log_cap + 1 : 0);
	L.log_sc = carve<float>(p, d.log_cap ? nq * d.log_cap + 1 : 0);
	L.log_cnt = carve<uint32_t>(p, d.log_cap ? nq : 0);
	L.log_slot = carve<uint32_t>(p, d.log_cap ? nq : 0);
	L.len = (size_t)(p - base);
	return L;
}
