/*
 * nxs_gpu_related.hip -- related terms (nxsgpu_related): for every query plan of a batch the dictionary terms
 * that occur in the docs the plan's expression matches (its doc set M, what "total" counts), with c = the docs
 * of M that hold the term and the live df, best k under the order of nxs_related.h, and how many are eligible --
 * exactly, however many.
 *
 * A PASS serves a group of G <= 32 distinct plans; bit g of a word stands for plan g.
 *
 *   k_rt_mask    the doc set as bits: one u32 per doc ordinal, bit g = "in M of plan g".  It is k_count_tile's
 *                body (count_tile_body<true>, nxs_gpu_dev.h) -- the range's presence masks in an LDS tile,
 *                truth table or postfix program -- with one more ending: an atomic OR of bit g into the words of
 *                the matching docs.  n = |M| is counted in the same sweep, as a total is.
 *   k_rt_scan    the hot kernel: ONE pass over d_post_dt per group.  A workgroup owns a fixed run of the flat
 *                posting array (NXS_GPU_RELATED_RUN postings) and finds the run's first term by a binary search
 *                of d_post_off.  A wavefront takes 64 postings at a time; each lane gathers the mask word of
 *                its posting's doc.  If no lane's word is set the wavefront moves on -- it has read 8 bytes a
 *                lane and nothing else.  Otherwise the lanes find their terms (one search for the wavefront
 *                when the 64 postings lie in one list), the segments of lanes that hold the same term are
 *                delimited by one ballot, and for every plan bit set in some lane one popcount of (ballot of
 *                the bit & segment) is added to c[g][term] by the segment's first lane: one atomic per
 *                (segment, bit), never one per posting.  A list that crosses a run or a wavefront boundary adds
 *                from both sides: integer sums, exact in any order.  No impact and no float is read.
 *   k_rt_select  grid (parts, plans): a plan's count row is cut into at most NXS_GPU_RELATED_PARTS parts of
 *                whole 256-term tiles.  A term that fails nxs_rt_eligible (mincount, mindf against the list's
 *                length, the plan's own <= 32 term ids) is skipped; the others are counted by ballot and feed a
 *                running top-k of nxs_rt_key in LDS (group_topk_take, shared with k_wc_match).
 *   k_rt_merge   one workgroup per plan: the k best of its parts (group_topk_merge, shared with k_wc_merge);
 *                c and df are read again at the winners.
 *
 * Device memory per pass: 4 bytes a doc (the masks), G x (terms + 1) x 4 bytes (the count rows, bounded by
 * NXS_GPU_RELATED_WS: G is what fits, 1 at least), G x parts x k keys.  Both are zeroed per pass
 * (hipMemsetAsync).  Identical plans of a batch are answered once and copied.  Plans that are empty, whose
 * ranking function scores nothing, whose positive lists are all empty or whose truth table accepts no mask
 * never reach the device: docs 0, no term.  The pass has a stream, grow-only workspace, pinned staging and
 * events of its own: beside batches and fuzzy passes in flight, none of their slots; blocking.  Nothing exists
 * until the first call.  Under NXS_GPU_RELATED=host the posting array is copied back, the doc set is evaluated
 * from the plan's postfix program (nxs_ds_eval, nxs_docset.h), the counts are taken by a plain loop over the lists and ranked by
 * nxs_rt_rank: the cross-check route.
 */
#include <string>
#include <unordered_map>

#include "nxs_gpu_int.h"
#include "nxs_gpu_dev.h"
#include "nxs_related.h"
#include "nxs_docset.h"

#define	RT_THREADS	256
#define	RT_GROUP_MAX	32u		/* plans per pass at most: the bits of a mask word */
#define	RT_PARTS_MAX	1024u		/* NXS_GPU_RELATED_PARTS at most (cfg_from_env) */
#define	RT_EVENTS	5

struct rt_q_t {
	uint32_t	n_excl;
	uint32_t	excl[NXS_RT_EXCL_MAX];
};

struct rt_state_t {
	side_t		side;
	double		prof[NXSGPU_RELATED_PROF];
};

__global__ void __launch_bounds__(CNT_THREADS)
k_rt_mask(const count_args_t A)
{
	count_tile_body<true>(A);
}

/* the term whose list holds position pos: the largest t in [lo, hi] with off[t] <= pos (off[lo] <= pos) */
static __device__ __forceinline__ uint32_t
rt_term_of(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t pos)
{
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo + 1) >> 1);

		if (off[mid] <= pos) {
			lo = mid;
		} else {
			hi = mid - 1;
		}
	}
	return lo;
}

__global__ void __launch_bounds__(RT_THREADS)
k_rt_scan(const uint64_t *__restrict__ post_off, const uint64_t *__restrict__ post_dt,
    const uint32_t *__restrict__ mask, uint64_t n_docs, uint32_t n_terms, uint64_t p_beg, uint64_t p_end, uint32_t run,
    uint32_t ng, uint32_t *cnt)
{
	__shared__ uint32_t s_t0;
	const unsigned tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
	const uint64_t r_beg = p_beg + (uint64_t)blockIdx.x * run;
	const uint64_t r_end = min(r_beg + run, p_end);

	if (r_beg >= r_end) {
		return;
	}
	if (tid == 0) {
		s_t0 = rt_term_of(post_off, 1, n_terms, r_beg);
	}
	__syncthreads();
	const uint32_t t0 = s_t0;

	for (uint64_t base = r_beg + (uint64_t)wid * WAVE; base < r_end; base += RT_THREADS) {
		const uint64_t pos = base + lane;
		const bool valid = pos < r_end;
		uint32_t m = 0;

		if (valid) {
			const uint64_t d = post_dt[pos] >> 32;

			if (d < n_docs) {
				m = mask[d];
			}
		}
		if (ballot64(m != 0) == 0) {
			continue;	/* no doc of any plan's set among these postings */
		}
		/* the lanes' terms: one search for the wavefront when its postings lie in one list */
		const uint32_t tb = rt_term_of(post_off, t0, n_terms, base);
		uint32_t t = 0;

		if (valid) {
			t = post_off[tb + 1] > pos ? tb : rt_term_of(post_off, tb, n_terms, pos);
		}
		/* segments of lanes with one term (lanes beyond the run: t = 0, m = 0, the last segment) */
		const uint32_t tprev = (uint32_t)__shfl_up((int)t, 1);
		const bool head = lane == 0 || t != tprev;
		const uint64_t heads = ballot64(head);
		const uint64_t above = lane == WAVE - 1 ? 0 : heads >> (lane + 1);
		const unsigned end = above ? lane + 1 + (unsigned)__builtin_ctzll(above) : WAVE;
		const uint64_t seg = (end == WAVE ? ~0ull : (1ull << end) - 1) & ~((1ull << lane) - 1);
		const bool adds = head && t >= 1 && t <= n_terms;

		for (uint32_t g = 0; g < ng; g++) {
			const uint64_t b = ballot64((m >> g) & 1u);

			if (b == 0) {
				continue;
			}
			const uint32_t c = (uint32_t)__popcll(b & seg);
			if (adds && c) {
				atomicAdd(&cnt[(size_t)g * ((size_t)n_terms + 1) + t], c);
			}
		}
	}
}

__global__ void __launch_bounds__(RT_THREADS)
k_rt_select(const uint64_t *__restrict__ post_off, const uint32_t *__restrict__ cnt, uint32_t n_terms,
    const rt_q_t *__restrict__ qs, int order, uint32_t mincount, uint32_t mindf, uint32_t np, uint32_t k,
    uint64_t *partial, uint32_t *matches)
{
	__shared__ uint64_t s_top[NXSGPU_RELATED_MAX];
	__shared__ uint64_t s_w[RT_THREADS / WAVE];
	__shared__ uint32_t s_flag[RT_THREADS / WAVE];
	__shared__ uint32_t s_cnt[RT_THREADS / WAVE];
	__shared__ uint32_t s_excl[NXS_RT_EXCL_MAX];
	__shared__ uint32_t s_nex;
	const uint32_t part = blockIdx.x, g = blockIdx.y;
	const unsigned tid = threadIdx.x, wid = tid / WAVE;
	const uint32_t tiles = (n_terms + RT_THREADS - 1) / RT_THREADS;
	const uint32_t t0 = (uint32_t)((uint64_t)part * tiles / np), t1 = (uint32_t)((uint64_t)(part + 1) * tiles / np);
	const uint32_t *__restrict__ row = cnt + (size_t)g * ((size_t)n_terms + 1);
	const uint64_t none = ~0ull;
	uint32_t wcnt = 0;

	if (tid < NXS_RT_EXCL_MAX) {
		s_excl[tid] = qs[g].excl[tid];
	}
	if (tid == 0) {
		s_nex = min(qs[g].n_excl, (uint32_t)NXS_RT_EXCL_MAX);
	}
	if (tid < NXSGPU_RELATED_MAX) {
		s_top[tid] = none;
	}
	__syncthreads();
	const uint32_t nex = s_nex;

	for (uint32_t tile = t0; tile < t1; tile++) {
		const uint32_t t = tile * RT_THREADS + tid + 1;
		uint64_t mine = none;
		bool hit = false;

		if (t <= n_terms) {
			const uint32_t c = row[t];

			if (c != 0) {
				const uint32_t len = (uint32_t)(post_off[t + 1] - post_off[t]);

				hit = nxs_rt_eligible(c, len, mincount, mindf, t, s_excl, nex);
				if (hit) {
					mine = nxs_rt_key(order, c, len, t);
				}
			}
		}
		wcnt += (uint32_t)__popcll(ballot64(hit));
		/* does some eligible key of this tile beat the k-th kept one? */
		const uint64_t beats = ballot64(hit && mine < s_top[k - 1]);
		if ((tid & (WAVE - 1)) == 0) {
			s_flag[wid] = beats != 0;
		}
		__syncthreads();
		if (s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3]) {
			group_topk_take<RT_THREADS>(mine, s_top, k, s_w, tid);
		}
		__syncthreads();
	}
	if ((tid & (WAVE - 1)) == 0) {
		s_cnt[wid] = wcnt;
	}
	__syncthreads();
	if (tid == 0) {
		const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];

		if (total) {
			atomicAdd(&matches[g], total);
		}
	}
	if (tid < k) {
		partial[((size_t)g * np + part) * k + tid] = s_top[tid];
	}
}

/* one workgroup per plan: the k smallest keys of its parts' lists, in order; c and df at the winners */
__global__ void __launch_bounds__(RT_THREADS)
k_rt_merge(const uint64_t *__restrict__ partial, uint32_t np, uint32_t k, const uint64_t *__restrict__ post_off,
    const uint32_t *__restrict__ cnt, uint32_t n_terms, uint32_t *term_ids, uint32_t *count, uint32_t *df,
    uint32_t *counts)
{
	__shared__ uint64_t s_w[RT_THREADS / WAVE];
	const uint32_t g = blockIdx.x;
	const unsigned tid = threadIdx.x;
	const uint64_t *list = partial + (size_t)g * np * k;
	const uint32_t *__restrict__ row = cnt + (size_t)g * ((size_t)n_terms + 1);
	const uint32_t nout = group_topk_merge<RT_THREADS>(list, np * k, k, s_w, tid, [&](uint32_t r, uint64_t best) {
		const uint32_t t = (uint32_t)best;
		const uint64_t at = (uint64_t)g * k + r;

		term_ids[at] = t;
		if (t >= 1 && t <= n_terms) {		/* (it is: the key came from this term) */
			count[at] = row[t];
			df[at] = (uint32_t)(post_off[t + 1] - post_off[t]);
		}
	});

	if (tid == 0) {
		counts[g] = nout;
	}
}

/* ------------------------------------------------------------------ */

void
rt_free(nxsgpu_index_t *ix)
{
	if (ix->rt) {
		side_close(&ix->rt->side, true);
		delete ix->rt;
		ix->rt = NULL;
	}
}

/* what a pass uploads (q | tok | prog | items | excl) and what it brings back (ids | c | df | counts | matches |
 * docs), the same layout in the staging area and on the device */
struct rt_layout_t {
	count_q_t *	q;
	uint64_t *	tok;
	uint8_t *	prog;
	count_item_t *	items;
	rt_q_t *	ex;
	size_t		up_len;
	uint32_t	*ids, *c, *df, *counts, *matches, *docs;
	size_t		out_off, out_len, len;
};

static rt_layout_t
rt_layout(uint8_t *base, uint32_t G, uint64_t items, uint32_t k)
{
	rt_layout_t L;
	uint8_t *p = base;

	L.q = carve<count_q_t>(p, G);
	L.tok = carve<uint64_t>(p, (size_t)G * 2 * NXSGPU_MAX_TOKENS);
	L.prog = carve<uint8_t>(p, (size_t)G * NXSGPU_MAX_PROG);
	L.items = carve<count_item_t>(p, items);
	L.ex = carve<rt_q_t>(p, G);
	L.up_len = (size_t)(p - base);
	L.ids = carve<uint32_t>(p, (size_t)G * k);
	L.out_off = (size_t)((uint8_t *)L.ids - base);
	L.c = carve<uint32_t>(p, (size_t)G * k);
	L.df = carve<uint32_t>(p, (size_t)G * k);
	L.counts = carve<uint32_t>(p, G);
	L.matches = carve<uint32_t>(p, G);
	L.docs = carve<uint32_t>(p, G);
	L.len = (size_t)(p - base);
	L.out_len = L.len - L.out_off;
	return L;
}

/* the posting range of a plan's token (beyond the snapshot's terms: no postings yet, like count_prepare) */
static inline void
rt_tok_range(const nxsgpu_index_t *ix, uint32_t tid, uint64_t *pb, uint64_t *pe)
{
	*pb = tid > ix->n_terms ? 0 : ix->h_post_off[tid];
	*pe = tid > ix->n_terms ? 0 : ix->h_post_off[(size_t)tid + 1];
}

/* the cross-check route for the distinct plans uq[0 .. nu): rows [nu][k] */
static int
rt_host(nxsgpu_index_t *ix, const nxsgpu_query_t *plans, const std::vector<uint32_t> &uq, int order, uint32_t mindf,
    uint32_t mincount, bool self, uint32_t k, uint32_t *u_ids, uint32_t *u_c, uint32_t *u_df, uint32_t *u_counts,
    uint32_t *u_matches, uint32_t *u_docs)
{
	const uint64_t P = ix->n_post, D = ix->n_docs;
	const uint32_t T = ix->n_terms;
	std::vector<uint64_t> h_dt(P);
	std::vector<uint32_t> pres(D), c((size_t)T + 1), df((size_t)T + 1);
	std::vector<uint8_t> in(D);
	hipStream_t st = ix->rt->side.st;

	if ((P && hipMemcpyAsync(h_dt.data(), ix->d_post_dt, P * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("related: copying the index back failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	for (uint32_t t = 1; t <= T; t++) {
		df[t] = (uint32_t)(ix->h_post_off[(size_t)t + 1] - ix->h_post_off[t]);
	}
	for (size_t u = 0; u < uq.size(); u++) {
		const nxsgpu_query_t &q = plans[uq[u]];
		uint64_t n = 0, matches = 0;

		std::fill(pres.begin(), pres.end(), 0u);
		for (uint32_t j = 0; j < q.n_tokens; j++) {
			uint64_t pb, pe;

			rt_tok_range(ix, q.term_id[j], &pb, &pe);
			for (uint64_t p = pb; p < pe; p++) {
				const uint64_t d = h_dt[p] >> 32;

				if (d < D) {
					pres[d] |= 1u << j;
				}
			}
		}
		for (uint64_t d = 0; d < D; d++) {
			in[d] = pres[d] != 0 && nxs_ds_eval(q.prog, q.prog_len, pres[d]);
			n += in[d];
		}
		std::fill(c.begin(), c.end(), 0u);
		for (uint32_t t = 1; t <= T; t++) {
			for (uint64_t p = ix->h_post_off[t]; p < ix->h_post_off[(size_t)t + 1]; p++) {
				const uint64_t d = h_dt[p] >> 32;

				c[t] += d < D && in[d];
			}
		}
		const int got = nxs_rt_rank(order, c.data(), df.data(), T, mincount, mindf, q.term_id, self ? 0 : q.n_tokens, k,
		    u_ids + u * k, &matches);
		if (got < 0) {
			set_error("related: out of memory");
			return -1;
		}
		for (int r = 0; r < got; r++) {
			const uint32_t t = u_ids[u * k + r];

			u_c[u * k + r] = c[t];
			u_df[u * k + r] = df[t];
		}
		u_counts[u] = (uint32_t)got;
		u_matches[u] = (uint32_t)matches;
		u_docs[u] = (uint32_t)n;
	}
	ix->rt->prof[1] += uq.size();
	return 0;
}

extern "C" int
nxsgpu_related(nxsgpu_index_t *ix, int algo, const nxsgpu_query_t *plans, uint32_t n, int order, uint32_t mindf,
    uint32_t mincount, int self, uint32_t k, uint32_t *term_ids, uint32_t *count, uint32_t *df, uint32_t *counts,
    uint32_t *matches, uint32_t *docs)
{
	if (algo != NXSGPU_BM25 && algo != NXSGPU_TF_IDF) {
		set_error("nxsgpu_related: unknown ranking function %d", algo);
		return -1;
	}
	if (k < 1 || k > NXSGPU_RELATED_MAX || mindf < 1 || mincount < 1 || (order != NXS_RT_COUNT && order != NXS_RT_SHARE)) {
		set_error("nxsgpu_related: k is 1..%d, mindf and mincount >= 1, order 0 or 1", NXSGPU_RELATED_MAX);
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	if (n > (1u << 24)) {
		set_error("nxsgpu_related: too many queries");
		return -1;
	}
	memset(term_ids, 0, (size_t)n * k * 4);
	memset(count, 0, (size_t)n * k * 4);
	memset(df, 0, (size_t)n * k * 4);
	memset(counts, 0, (size_t)n * 4);
	memset(matches, 0, (size_t)n * 4);
	memset(docs, 0, (size_t)n * 4);

	const uint32_t T = ix->n_terms;
	const uint64_t D = ix->n_docs;
	const bool valid = (algo == NXSGPU_BM25) ? ix->bm25_valid : ix->tfidf_valid;

	if (ix->h_post_off.size() < (size_t)T + 2 || ix->h_post_off[(size_t)T + 1] > ix->n_post || D > 0xfffffffeull) {
		set_error("nxsgpu_related: inconsistent row offsets");
		return -1;
	}
	/* the distinct plans that have work to do, in the order they were first met */
	std::vector<uint32_t> uq, rep(n, ~0u);
	std::unordered_map<std::string, uint32_t> seen;

	for (uint32_t i = 0; i < n; i++) {
		const nxsgpu_query_t &q = plans[i];
		uint64_t sum = 0;

		if (q.n_tokens > NXSGPU_MAX_TOKENS || q.prog_len > NXSGPU_MAX_PROG) {
			set_error("query %u exceeds the device limits", i);
			return -1;
		}
		if (!valid || q.n_tokens == 0 || D == 0 || T == 0) {
			continue;
		}
		/* (the program is evaluated above 8 tokens, and for every plan on the host route) */
		if ((q.n_tokens > 8 || ix->cfg.related_host) && !nxs_ds_prog_ok(q.prog, q.prog_len, q.n_tokens)) {
			set_error("query %u: a malformed postfix program, or one deeper than 64", i);
			return -1;
		}
		for (uint32_t j = 0; j < q.n_tokens; j++) {
			uint64_t pb, pe;

			if (q.term_id[j] == 0) {
				set_error("query %u: bad term id 0", i);
				return -1;
			}
			rt_tok_range(ix, q.term_id[j], &pb, &pe);
			sum += pe - pb;
		}
		if (sum == 0) {
			continue;
		}
		if (q.n_tokens <= 8) {
			bool any = false;

			for (uint32_t m = 1; m < (1u << q.n_tokens) && !any; m++) {
				any = (q.truth[m >> 5] >> (m & 31)) & 1;
			}
			if (!any) {
				continue;
			}
		}
		const auto at = seen.emplace(std::string((const char *)&q, sizeof(q)), (uint32_t)uq.size());
		if (at.second) {
			uq.push_back(i);
		}
		rep[i] = at.first->second;
	}
	const uint32_t nu = (uint32_t)uq.size();
	if (nu == 0) {
		return 0;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	if (!ix->rt) {
		ix->rt = new rt_state_t();
	}
	rt_state_t *rt = ix->rt;
	side_t *sd = &rt->side;

	if (side_open(ix, sd, "related", RT_EVENTS, true) != 0) {
		return -1;
	}
	hipStream_t st = sd->st;
	const bool prof = ix->profiling && sd->ev_ok;
	std::vector<uint32_t> u_ids((size_t)nu * k, 0), u_c((size_t)nu * k, 0), u_df((size_t)nu * k, 0), u_counts(nu, 0),
	    u_matches(nu, 0), u_docs(nu, 0);

	rt->prof[7] += 1;
	if (ix->cfg.related_host) {
		if (rt_host(ix, plans, uq, order, mindf, mincount, self != 0, k, u_ids.data(), u_c.data(), u_df.data(),
		    u_counts.data(), u_matches.data(), u_docs.data()) != 0) {
			return -1;
		}
	} else {
		const size_t row = ((size_t)T + 1) * 4;
		const uint32_t G = (uint32_t)std::min<uint64_t>(std::min(RT_GROUP_MAX, nu), std::max<uint64_t>(1, ix->cfg.related_ws / row));
		const uint32_t tiles = (T + RT_THREADS - 1) / RT_THREADS;
		const uint32_t np = std::max<uint32_t>(1, std::min(std::min(ix->cfg.related_parts, RT_PARTS_MAX), tiles));
		const uint32_t run = std::max<uint32_t>(WAVE, ix->cfg.related_run / WAVE * WAVE);
		const uint64_t p_beg = ix->h_post_off[1], p_end = ix->h_post_off[(size_t)T + 1];
		const uint64_t items8 = (D + CNT_TILE8_DOCS - 1) / CNT_TILE8_DOCS, items32 = (D + CNT_TILE32_DOCS - 1) / CNT_TILE32_DOCS;
		const uint64_t n_runs = (p_end - p_beg + run - 1) / run;

		if ((uint64_t)G * items32 > 0x7fffffffull || n_runs > 0x7fffffffull) {
			set_error("related plan too large");
			return -1;
		}
		const rt_layout_t L0 = rt_layout(NULL, G, (uint64_t)G * items32, k);
		const size_t o_mask = (L0.len + 255) & ~(size_t)255, o_cnt = o_mask + ((D * 4 + 255) & ~(size_t)255);
		const size_t o_part = o_cnt + (((size_t)G * row + 255) & ~(size_t)255);
		const size_t ws_need = o_part + (size_t)G * np * k * 8 + 512;

		if (side_room(sd, "related", L0.len + 512, ws_need) != 0) {
			return -1;
		}
		uint8_t *h = (uint8_t *)(((uintptr_t)sd->pin + 255) & ~(uintptr_t)255);
		uint8_t *d = (uint8_t *)(((uintptr_t)sd->ws + 255) & ~(uintptr_t)255);
		uint32_t *d_mask = (uint32_t *)(d + o_mask), *d_cnt = (uint32_t *)(d + o_cnt);
		uint64_t *d_part = (uint64_t *)(d + o_part);

		for (uint32_t u0 = 0; u0 < nu; u0 += G) {
			const uint32_t m = std::min(G, nu - u0);
			const rt_layout_t H = rt_layout(h, G, (uint64_t)G * items32, k), Dv = rt_layout(d, G, (uint64_t)G * items32, k);
			uint32_t n_items = 0;

			memset(h, 0, H.up_len);
			for (uint32_t g = 0; g < m; g++) {
				const nxsgpu_query_t &q = plans[uq[u0 + g]];
				count_q_t &c = H.q[g];
				const uint64_t ni = q.n_tokens <= 8 ? items8 : items32;

				c.nt = q.n_tokens;
				c.prog_len = q.prog_len;
				c.out = g;
				c.tok_base = g * 2 * NXSGPU_MAX_TOKENS;
				c.prog_base = g * NXSGPU_MAX_PROG;
				memcpy(c.truth, q.truth, sizeof(c.truth));
				for (uint32_t j = 0; j < q.n_tokens; j++) {
					rt_tok_range(ix, q.term_id[j], &H.tok[c.tok_base + 2 * j], &H.tok[c.tok_base + 2 * j + 1]);
				}
				memcpy(H.prog + c.prog_base, q.prog, q.prog_len);
				for (uint64_t r = 0; r < ni; r++) {
					H.items[n_items].q = g;
					H.items[n_items++].r = (uint32_t)r;
				}
				H.ex[g].n_excl = self ? 0 : q.n_tokens;
				memcpy(H.ex[g].excl, q.term_id, sizeof(uint32_t) * q.n_tokens);
			}
			if (hipMemcpyAsync(d, h, H.up_len, hipMemcpyHostToDevice, st) != hipSuccess ||
			    hipMemsetAsync(d + Dv.out_off, 0, Dv.out_len, st) != hipSuccess ||
			    hipMemsetAsync(d_mask, 0, D * 4, st) != hipSuccess ||
			    hipMemsetAsync(d_cnt, 0, (size_t)m * row, st) != hipSuccess) {
				set_error("related upload failed");
				(void)hipStreamSynchronize(st);
				return -1;
			}
			count_args_t a;

			a.post_dt = ix->d_post_dt;
			a.q = Dv.q;
			a.tok = Dv.tok;
			a.prog = Dv.prog;
			a.items = Dv.items;
			a.n_docs = D;
			a.totals = Dv.docs;
			a.mask = d_mask;
			if (prof) (void)hipEventRecord(sd->ev[0], st);
			hipLaunchKernelGGL(k_rt_mask, dim3(n_items), dim3(CNT_THREADS), 0, st, a);
			if (prof) (void)hipEventRecord(sd->ev[1], st);
			if (n_runs) {
				hipLaunchKernelGGL(k_rt_scan, dim3((uint32_t)n_runs), dim3(RT_THREADS), 0, st, ix->d_post_off, ix->d_post_dt,
				    (const uint32_t *)d_mask, D, T, p_beg, p_end, run, m, d_cnt);
			}
			if (prof) (void)hipEventRecord(sd->ev[2], st);
			hipLaunchKernelGGL(k_rt_select, dim3(np, m), dim3(RT_THREADS), 0, st, ix->d_post_off, (const uint32_t *)d_cnt, T,
			    (const rt_q_t *)Dv.ex, order, mincount, mindf, np, k, d_part, Dv.matches);
			if (prof) (void)hipEventRecord(sd->ev[3], st);
			hipLaunchKernelGGL(k_rt_merge, dim3(m), dim3(RT_THREADS), 0, st, (const uint64_t *)d_part, np, k, ix->d_post_off,
			    (const uint32_t *)d_cnt, T, Dv.ids, Dv.c, Dv.df, Dv.counts);
			if (prof) (void)hipEventRecord(sd->ev[4], st);
			if (hipGetLastError() != hipSuccess) {
				set_error("related kernel launch failed");
				(void)hipStreamSynchronize(st);
				return -1;
			}
			if (hipMemcpyAsync(h + H.out_off, d + Dv.out_off, H.out_len, hipMemcpyDeviceToHost, st) != hipSuccess ||
			    hipStreamSynchronize(st) != hipSuccess) {
				set_error("related pass failed: %s", hipGetErrorString(hipGetLastError()));
				return -1;
			}
			memcpy(u_ids.data() + (size_t)u0 * k, H.ids, (size_t)m * k * 4);
			memcpy(u_c.data() + (size_t)u0 * k, H.c, (size_t)m * k * 4);
			memcpy(u_df.data() + (size_t)u0 * k, H.df, (size_t)m * k * 4);
			memcpy(u_counts.data() + u0, H.counts, (size_t)m * 4);
			memcpy(u_matches.data() + u0, H.matches, (size_t)m * 4);
			memcpy(u_docs.data() + u0, H.docs, (size_t)m * 4);
			if (prof) {
				for (int e = 0; e < 4; e++) {
					rt->prof[3 + e] += side_elapsed(sd, e, e + 1);
				}
			}
			rt->prof[0] += m;
			rt->prof[2] += 1;
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t u = rep[i];

		if (u == ~0u) {
			continue;
		}
		memcpy(term_ids + (size_t)i * k, u_ids.data() + (size_t)u * k, (size_t)k * 4);
		memcpy(count + (size_t)i * k, u_c.data() + (size_t)u * k, (size_t)k * 4);
		memcpy(df + (size_t)i * k, u_df.data() + (size_t)u * k, (size_t)k * 4);
		counts[i] = std::min(u_counts[u], k);
		matches[i] = u_matches[u];
		docs[i] = u_docs[u];
	}
	return 0;
}

extern "C" void
nxsgpu_related_profile(nxsgpu_index_t *ix, double out[NXSGPU_RELATED_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_RELATED_PROF);
	if (ix->rt) {
		memcpy(out, ix->rt->prof, sizeof(ix->rt->prof));
		if (reset) {
			memset(ix->rt->prof, 0, sizeof(ix->rt->prof));
		}
	}
}
