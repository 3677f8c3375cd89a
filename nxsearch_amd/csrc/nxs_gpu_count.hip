/*
 * nxs_gpu_count.hip -- k_count_tile / k_count_req + nxsgpu_count: total match counts
 * (MI355X / gfx950 query path of nxsearch; see nxs_gpu_int.h for the map of the files)
 *
 * total of a query = cardinality of the reference's expression bitmap (get_expr_bitmap,
 * search.c:118-174).  The top-k kernels avoid most matching docs on purpose, so the count
 * is a pass of its own.  It needs the doc ordinals and the truth table, nothing else: it
 * reads the primary CSR (nxsgpu_index::d_post_dt, ordinal in the high word -- the same
 * array for every ranking function, untouched by the outlier lists of the TF-IDF dense
 * terms) through the terms' ORIGINAL posting ranges, and sums integers (any order).
 *
 *  k_count_tile  one workgroup per (query, doc range): presence masks of the range in
 *                an LDS tile (bytes up to 8 tokens, words up to 32), filled by LDS atomics,
 *                evaluated by truth table / postfix program, counted by ballot
 *  k_count_req   queries with a required token: one lane per posting of the SHORTEST
 *                required list, membership in the other lists by bisection inside the
 *                span of the workgroup's driver window -- no tile, work proportional to
 *                that list
 *
 * Each workgroup ends in at most ONE global atomicAdd into totals[query].
 */
#include "nxs_gpu_int.h"
#include "nxs_gpu_dev.h"

#define	CNT_REQ_CHUNK	2048				/* driver postings per workgroup */

/* (the tile's body -- count_q_t, count_args_t, count_tile_body -- is nxs_gpu_dev.h's: k_rt_mask shares it) */
__global__ void __launch_bounds__(CNT_THREADS)
k_count_tile(const count_args_t A)
{
	count_tile_body<false>(A);
}

__global__ void __launch_bounds__(CNT_THREADS)
k_count_req(const count_args_t A)
{
	__shared__ uint64_t s_lo[8], s_hi[8];
	__shared__ uint32_t s_truth[8];
	__shared__ uint32_t s_cnt;

	const unsigned tid = threadIdx.x;
	const count_item_t it = A.items[blockIdx.x];
	const count_q_t Q = A.q[it.q];
	const uint64_t *__restrict__ dt = A.post_dt;
	const uint32_t D = Q.driver;
	const uint64_t db = A.tok[Q.tok_base + 2 * D] + (uint64_t)it.r * CNT_REQ_CHUNK;
	const uint64_t de = min(db + CNT_REQ_CHUNK, A.tok[Q.tok_base + 2 * D + 1]);

	if (db >= de) {
		return;
	}
	if (tid == 0) {
		s_cnt = 0;
	}
	if (tid < 8) {
		s_truth[tid] = Q.truth[tid];
	}
	/* the span of the driver window in every other list */
	if (tid < Q.nt) {
		const uint64_t first = dt[db] >> 32, last = dt[de - 1] >> 32;
		const uint64_t pb = A.tok[Q.tok_base + 2 * tid], pe = A.tok[Q.tok_base + 2 * tid + 1];
		const uint64_t lo = dt_lower_bound(dt, pb, pe, first);
		s_lo[tid] = lo;
		s_hi[tid] = dt_lower_bound(dt, lo, pe, last + 1);
	}
	__syncthreads();

	uint32_t n = 0;		/* wavefront-uniform */
	for (uint64_t base = db; base < de; base += CNT_THREADS) {
		const uint64_t i = base + tid;
		bool match = false;
		if (i < de) {
			const uint64_t d = dt[i] >> 32;
			uint32_t m = 1u << D;
			for (uint32_t t = 0; t < Q.nt; t++) {
				if (t == D) {
					continue;
				}
				const uint64_t hi = s_hi[t];
				const uint64_t p = dt_lower_bound(dt, s_lo[t], hi, d);
				if (p < hi && (dt[p] >> 32) == d) {
					m |= 1u << t;
				} else if ((Q.req >> t) & 1u) {
					break;		/* a required token is missing: no mask with it matches */
				}
			}
			match = (s_truth[m >> 5] >> (m & 31)) & 1u;
		}
		n += (uint32_t)__popcll(ballot64(match));
	}
	if ((tid & (WAVE - 1)) == 0 && n) {
		atomicAdd(&s_cnt, n);
	}
	__syncthreads();
	if (tid == 0 && s_cnt) {
		atomicAdd(&A.totals[Q.out], s_cnt);
	}
}

/* ------------------------------------------------------------------ */

extern "C" void
nxsgpu_count_tile_widths(uint32_t out[2])
{
	out[0] = CNT_TILE8_DOCS;
	out[1] = CNT_TILE32_DOCS;
}

void
count_buf_free(count_buf_t &cb)
{
	(void)hipFree(cb.d);
	if (cb.h) {
		(void)hipHostFree(cb.h);
	}
	for (int i = 0; i < 3; i++) {
		if (cb.ev_k[i]) {
			(void)hipEventDestroy(cb.ev_k[i]);
		}
	}
	memset(&cb, 0, sizeof(cb));
}

/* the plan's arrays, the same layout in the staging area and on the device */
struct count_layout_t {
	uint32_t *	totals;		/* the blocking call's own (a batch's live in its batch_layout_t) */
	count_q_t *	q;
	uint64_t *	tok;
	uint8_t *	prog;
	count_item_t *	tile_items, *req_items;
	size_t		len;
};

static count_layout_t
count_layout(uint8_t *base, const count_buf_t &cb)
{
	count_layout_t L;
	uint8_t *p = base;

	L.totals = carve<uint32_t>(p, cb.n_tot);
	L.q = carve<count_q_t>(p, cb.n_q);
	L.tok = carve<uint64_t>(p, cb.n_tok);
	L.prog = carve<uint8_t>(p, cb.n_prog);
	L.tile_items = carve<count_item_t>(p, cb.n_tile);
	L.req_items = carve<count_item_t>(p, cb.n_req);
	L.len = (size_t)(p - base);
	return L;
}

/*
 * Routing (NXS_GPU_COUNT=auto): a query that resolves to nothing, whose ranking function
 * scores nothing (ranking.c:86-88,156-166) or whose truth table accepts no mask is 0; a
 * single positive token is its list's length; a query with a required token takes the
 * driver kernel (its work is the shortest required list).  Everything else takes the exact
 * path's count pass (count_scan_pass), NOT k_count_tile: measured on C3's OR half the tile
 * kernel lost to that pass (5.6 against 2.2 ms per 512 queries, NOTES.md) -- it stays behind
 * NXS_GPU_COUNT=tile until it is shown to win.
 */
int
count_prepare(nxsgpu_index_t *ix, int algo, const nxsgpu_query_t *queries, uint32_t nq, count_buf_t &cb,
    uint32_t *h_totals, bool own_totals, bool own_streams)
{
	std::vector<uint32_t> by_scan;	/* auto: the queries the exact path's count pass takes */
	const bool valid = (algo == NXSGPU_BM25) ? ix->bm25_valid : ix->tfidf_valid;
	const uint32_t mode = ix->cfg.count_mode;
	std::vector<count_q_t> cq;
	std::vector<uint64_t> tok;
	std::vector<uint8_t> prog;
	std::vector<count_item_t> tile_items, req_items;

	cb.up_len = 0;
	cb.n_tile = cb.n_req = cb.q_tile = cb.q_req = 0;
	cb.n_q = cb.n_tok = cb.n_prog = cb.n_tot = 0;
	cb.timed = false;
	for (uint32_t i = 0; i < nq; i++) {
		const nxsgpu_query_t &q = queries[i];
		count_q_t c;
		uint64_t pb[NXSGPU_MAX_TOKENS], pe[NXSGPU_MAX_TOKENS], sum = 0;

		h_totals[i] = 0;
		if (q.n_tokens > NXSGPU_MAX_TOKENS || q.prog_len > NXSGPU_MAX_PROG) {
			set_error("query %u exceeds the device limits", i);
			return -1;
		}
		if (!valid || q.n_tokens == 0) {
			continue;
		}
		memset(&c, 0, sizeof(c));
		c.nt = q.n_tokens;
		c.prog_len = q.prog_len;
		c.out = i;
		for (uint32_t t = 0; t < c.nt; t++) {
			const uint32_t tid = q.term_id[t];
			if (tid == 0) {
				set_error("query %u: bad term id 0", i);
				return -1;
			}
			/* (beyond the snapshot's terms: no postings yet, like fill_dev_chunk) */
			pb[t] = tid > ix->n_terms ? 0 : ix->h_post_off[tid];
			pe[t] = tid > ix->n_terms ? 0 : ix->h_post_off[tid + 1];
			sum += pe[t] - pb[t];
		}
		if (sum == 0) {
			continue;
		}
		if (c.nt <= 8) {
			uint32_t r = (1u << c.nt) - 1;
			bool any = false;
			memcpy(c.truth, q.truth, sizeof(c.truth));
			for (uint32_t m = 1; m < (1u << c.nt); m++) {
				if ((c.truth[m >> 5] >> (m & 31)) & 1) {
					r &= m;
					any = true;
				}
			}
			if (!any) {
				continue;
			}
			c.req = r;
		}
		if (c.nt == 1 && mode == COUNT_AUTO) {
			h_totals[i] = (uint32_t)(pe[0] - pb[0]);	/* a single positive token: its list */
			continue;
		}
		const bool by_req = c.req != 0 && mode != COUNT_TILE;
		if (!by_req && mode == COUNT_AUTO) {
			by_scan.push_back(i);
			continue;
		}
		if (by_req) {
			uint32_t drv = 0;
			uint64_t best = ~0ull;
			for (uint32_t t = 0; t < c.nt; t++) {
				if (((c.req >> t) & 1) && pe[t] - pb[t] < best) {
					best = pe[t] - pb[t];
					drv = t;
				}
			}
			if (best == 0) {
				continue;	/* a required token is in no doc */
			}
			c.driver = drv;
		}
		if ((uint64_t)tok.size() + 2 * c.nt > 0xffffffffull || (uint64_t)prog.size() + c.prog_len > 0xffffffffull) {
			set_error("count plan too large");
			return -1;
		}
		c.tok_base = (uint32_t)tok.size();
		for (uint32_t t = 0; t < c.nt; t++) {
			tok.push_back(pb[t]);
			tok.push_back(pe[t]);
		}
		if (c.nt > 8) {
			c.prog_base = (uint32_t)prog.size();
			prog.insert(prog.end(), q.prog, q.prog + q.prog_len);
		}
		const uint32_t qi = (uint32_t)cq.size();
		uint64_t n_items;
		if (by_req) {
			n_items = (pe[c.driver] - pb[c.driver] + CNT_REQ_CHUNK - 1) / CNT_REQ_CHUNK;
		} else {
			const uint64_t W = c.nt <= 8 ? CNT_TILE8_DOCS : CNT_TILE32_DOCS;
			n_items = (ix->n_docs + W - 1) / W;
		}
		std::vector<count_item_t> &items = by_req ? req_items : tile_items;
		if (items.size() + n_items > 0x7fffffffull) {
			set_error("count plan too large");
			return -1;
		}
		for (uint64_t r = 0; r < n_items; r++) {
			count_item_t it;
			it.q = qi;
			it.r = (uint32_t)r;
			items.push_back(it);
		}
		(by_req ? cb.q_req : cb.q_tile)++;
		cq.push_back(c);
	}
	if (!by_scan.empty()) {
		/* blocking, before anything of this count is queued: their totals go up with the host-known ones */
		std::vector<nxsgpu_query_t> sub(by_scan.size());
		std::vector<uint32_t> st(by_scan.size());
		for (size_t j = 0; j < by_scan.size(); j++) {
			sub[j] = queries[by_scan[j]];
		}
		if (count_scan_pass(ix, algo, sub.data(), (uint32_t)sub.size(), st.data(), own_streams) != 0) {
			return -1;
		}
		for (size_t j = 0; j < by_scan.size(); j++) {
			h_totals[by_scan[j]] = st[j];
		}
	}
	if (cq.empty()) {
		return 0;
	}
	cb.n_q = (uint32_t)cq.size();
	cb.n_tok = (uint32_t)tok.size();
	cb.n_prog = (uint32_t)prog.size();
	cb.n_tot = own_totals ? nq : 0;
	cb.n_tile = (uint32_t)tile_items.size();
	cb.n_req = (uint32_t)req_items.size();
	const size_t need = count_layout(NULL, cb).len + 4096;
	if (cb.h_len < need) {
		if (cb.h) {
			(void)hipHostFree(cb.h);
		}
		cb.h = NULL;
		cb.h_len = 0;
		const size_t len = (need + (size_t(1) << 20)) & ~((size_t(1) << 20) - 1);
		if (hipHostMalloc((void **)&cb.h, len, hipHostMallocDefault) != hipSuccess) {
			set_error("hipHostMalloc(%zu) failed", len);
			return -1;
		}
		cb.h_len = len;
	}
	if (cb.d_len < need) {
		(void)hipFree(cb.d);
		cb.d = NULL;
		cb.d_len = 0;
		const size_t len = (need + (size_t(1) << 20)) & ~((size_t(1) << 20) - 1);
		if (hipMalloc(&cb.d, len) != hipSuccess) {
			set_error("hipMalloc(%zu) for the count plan failed", len);
			return -1;
		}
		cb.d_len = len;
	}
	const count_layout_t H = count_layout(cb.h, cb);
	if (own_totals) {
		memcpy(H.totals, h_totals, (size_t)nq * 4);
	}
	memcpy(H.q, cq.data(), cq.size() * sizeof(count_q_t));
	memcpy(H.tok, tok.data(), tok.size() * 8);
	if (!prog.empty()) {
		memcpy(H.prog, prog.data(), prog.size());
	}
	if (!tile_items.empty()) {
		memcpy(H.tile_items, tile_items.data(), tile_items.size() * sizeof(count_item_t));
	}
	if (!req_items.empty()) {
		memcpy(H.req_items, req_items.data(), req_items.size() * sizeof(count_item_t));
	}
	cb.up_len = H.len;
	return 0;
}

int
count_launch(nxsgpu_index_t *ix, count_buf_t &cb, uint32_t *d_totals, hipStream_t st)
{
	if (cb.up_len == 0 || (cb.n_tile == 0 && cb.n_req == 0)) {
		return 0;
	}
	const count_layout_t D = count_layout((uint8_t *)cb.d, cb);
	count_args_t a;

	if (hipMemcpyAsync(cb.d, cb.h, cb.up_len, hipMemcpyHostToDevice, st) != hipSuccess) {
		set_error("count plan upload failed");
		return -1;
	}
	a.post_dt = ix->d_post_dt;	/* (the CSR that is current now: a refresh swaps the buffer) */
	a.q = D.q;
	a.tok = D.tok;
	a.prog = D.prog;
	a.n_docs = ix->n_docs;
	a.totals = d_totals ? d_totals : D.totals;
	a.mask = NULL;
	cb.timed = false;
	if (ix->profiling) {
		bool ok = true;
		for (int i = 0; i < 3 && ok; i++) {
			ok = cb.ev_k[i] || hipEventCreate(&cb.ev_k[i]) == hipSuccess;
		}
		cb.timed = ok;
	}
	if (cb.timed) (void)hipEventRecord(cb.ev_k[0], st);
	if (cb.n_tile) {
		a.items = D.tile_items;
		hipLaunchKernelGGL(k_count_tile, dim3(cb.n_tile), dim3(CNT_THREADS), 0, st, a);
	}
	if (cb.timed) (void)hipEventRecord(cb.ev_k[1], st);
	if (cb.n_req) {
		a.items = D.req_items;
		hipLaunchKernelGGL(k_count_req, dim3(cb.n_req), dim3(CNT_THREADS), 0, st, a);
	}
	if (cb.timed) (void)hipEventRecord(cb.ev_k[2], st);
	if (hipGetLastError() != hipSuccess) {
		set_error("count kernel launch failed");
		return -1;
	}
	return 1;
}

void
count_collect(nxsgpu_index_t *ix, count_buf_t &cb)
{
	if (!cb.timed) {
		return;
	}
	cb.timed = false;
	float a = 0, b = 0;
	if (hipEventElapsedTime(&a, cb.ev_k[0], cb.ev_k[1]) != hipSuccess ||
	    hipEventElapsedTime(&b, cb.ev_k[1], cb.ev_k[2]) != hipSuccess) {
		(void)hipGetLastError();
		return;
	}
	if (cb.n_tile) {
		ix->cnt_prof[0] += 1;
		ix->cnt_prof[1] += a;
		ix->cnt_prof[4] += cb.q_tile;
	}
	if (cb.n_req) {
		ix->cnt_prof[2] += 1;
		ix->cnt_prof[3] += b;
		ix->cnt_prof[5] += cb.q_req;
	}
}

extern "C" void
nxsgpu_count_profile(nxsgpu_index_t *ix, double out[6], int reset)
{
	memcpy(out, ix->cnt_prof, sizeof(ix->cnt_prof));
	if (reset) {
		memset(ix->cnt_prof, 0, sizeof(ix->cnt_prof));
	}
}

extern "C" int
nxsgpu_count(nxsgpu_index_t *ix, int algo, const nxsgpu_query_t *queries, uint32_t nq, uint32_t *totals)
{
	/* (beside batches in flight: on the blocking search's stream, like nxsgpu_search) */
	const hipStream_t st = nxsgpu_batches_in_flight(ix) ? ix->xstream[0] : ix->stream;
	count_buf_t &cb = ix->cnt_blk;
	int rc = 0;

	if (algo != NXSGPU_BM25 && algo != NXSGPU_TF_IDF) {
		set_error("invalid algorithm");
		return -1;
	}
	if (nq == 0) {
		return 0;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	if (ix->cfg.count_mode == COUNT_SCAN) {
		return count_scan_pass(ix, algo, queries, nq, totals, true);
	}
	/* (the totals go up with what the host knows of them; the kernels add the rest) */
	if (count_prepare(ix, algo, queries, nq, cb, totals, true, true) != 0) {
		return -1;
	}
	const int lr = count_launch(ix, cb, NULL, st);
	if (lr == 0) {
		return 0;
	}
	const count_layout_t H = count_layout(cb.h, cb), D = count_layout((uint8_t *)cb.d, cb);
	if (lr < 0) {
		rc = -1;
	} else if (hipMemcpyAsync(H.totals, D.totals, (size_t)nq * 4, hipMemcpyDeviceToHost, st) != hipSuccess) {
		set_error("count pass: copy failed");
		rc = -1;
	}
	if (hipStreamSynchronize(st) != hipSuccess) {
		set_error("count pass failed: %s", hipGetErrorString(hipGetLastError()));
		rc = -1;
	}
	if (rc == 0) {
		memcpy(totals, H.totals, (size_t)nq * 4);
		count_collect(ix, cb);
	}
	return rc;
}
