/*
 * nxs_gpu_matchdocs.hip -- a query's matches listed by doc id (nxsgpu_match_docs): for every (plan, cursor) pair of a
 * batch the docs of the plan's doc set M (what "total" counts, what the related pass calls M) whose id is >= the
 * cursor, in ascending doc id, the first `limit` of them, with |M| and whether a doc of M lies beyond the page.
 *
 * Doc ordinals ascend with doc ids, so a page is a stream compaction of M's bits from the cursor's ordinal on.
 * A PASS serves a group of G <= 32 distinct pairs; bit g of a mask word stands for pair g.
 *
 *   k_md_mask    the doc sets as bits, one u32 per doc ordinal: count_tile_body<true> (nxs_gpu_dev.h), the body
 *                of k_count_tile and k_rt_mask, unedited.  totals[g] = |M| comes from the same sweep.
 *   k_md_from    a lane per pair: the cursor as an ordinal (nxs_md_lower_bound over d_doc_ids, nxs_matchdocs.h).
 *   k_md_count   the ordinals are cut into runs of NXS_GPU_MATCHDOCS_RUN, a wavefront per run.  A lane reads the
 *                mask word of its ordinal; for every pair bit g one ballot of (bit set and ordinal >= from_ord[g])
 *                and a popcount, kept by lane g.  One plain store per (g, run) into run_cnt[g][run]: no atomic, and
 *                every cell is written, so the rows need no memset.
 *   k_md_scan    a workgroup per pair: the exclusive prefix sum of its row in place, in chunks of 256 with a
 *                carry; the row's sum goes into run_cnt[g][n_runs], more[g] = sum > limit, counts[g] = min(sum,
 *                limit).  Sums fit u32 (D <= 0xfffffffe).
 *   k_md_emit    the same runs again.  Lane g holds the running base of pair g.  A wavefront whose base is >= limit
 *                or whose run holds nothing, for every pair, leaves after reading those.  Otherwise a lane's rank is
 *                the base plus the popcount of the ballot below the lane, and a lane with rank < limit stores
 *                d_doc_ids[ordinal] into ids[g][rank].  Ascending and deterministic by construction.
 *
 * Device memory per pass: 4 bytes a doc (the masks, zeroed per pass), 4 bytes per (pair, run + 1), 8 x cap bytes
 * per pair (cap = min(limit, D)), bounded by NXS_GPU_MATCHDOCS_WS: G is what fits, 1 at least.  Identical (plan,
 * cursor) pairs of a batch are answered once and copied.  Plans that are empty, whose ranking function scores
 * nothing, whose lists are all empty or whose truth table accepts no mask never reach the device.  The counts
 * come back first (one small copy), then counts[g] ids per pair straight into the caller's rows: the length of the
 * second step is not known before the first.  The pass has a stream, grow-only workspace, pinned staging and
 * events of its own: beside batches and fuzzy passes in flight, none of their slots; blocking.  Nothing exists
 * until the first call.  No impact is read, so nothing is materialised.  Under NXS_GPU_MATCHDOCS=host d_post_dt
 * and d_doc_ids are copied back, M is evaluated from the plan's postfix program over presence masks (nxs_ds_eval,
 * as the related pass's host route does) and the page is nxs_md_page's: the cross-check route.
 */
#include <string>
#include <unordered_map>

#include "nxs_gpu_int.h"
#include "nxs_gpu_dev.h"
#include "nxs_docset.h"
#include "nxs_matchdocs.h"

#define	MD_THREADS	256
#define	MD_WAVES	(MD_THREADS / WAVE)
#define	MD_GROUP_MAX	32u		/* pairs per pass at most: the bits of a mask word */
#define	MD_EVENTS	6

struct md_state_t {
	side_t		side;
	double		prof[NXSGPU_MATCHDOCS_PROF];
};

__global__ void __launch_bounds__(CNT_THREADS)
k_md_mask(const count_args_t A)
{
	count_tile_body<true>(A);
}

__global__ void __launch_bounds__(WAVE)
k_md_from(const uint64_t *__restrict__ doc_ids, uint64_t n_docs, const uint64_t *__restrict__ from, uint32_t ng,
    uint32_t *from_ord)
{
	const unsigned g = threadIdx.x;

	if (g < ng) {
		from_ord[g] = (uint32_t)nxs_md_lower_bound(doc_ids, n_docs, from[g]);
	}
}

/* run_cnt: [ng][n_runs + 1]; cell (g, r) = the docs of pair g's set at or beyond its cursor in run r */
__global__ void __launch_bounds__(MD_THREADS)
k_md_count(const uint32_t *__restrict__ mask, uint64_t n_docs, uint32_t run, uint32_t n_runs,
    const uint32_t *__restrict__ from_ord, uint32_t ng, uint32_t *run_cnt)
{
	__shared__ uint32_t s_from[MD_GROUP_MAX];
	const unsigned tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;

	if (tid < MD_GROUP_MAX) {
		s_from[tid] = tid < ng ? from_ord[tid] : 0xffffffffu;
	}
	__syncthreads();
	const uint64_t r = (uint64_t)blockIdx.x * MD_WAVES + wid;

	if (r >= n_runs) {
		return;
	}
	const uint64_t o_beg = r * run, o_end = min(o_beg + run, n_docs);
	uint32_t c = 0;		/* lane g: pair g's count */

	for (uint64_t base = o_beg; base < o_end; base += WAVE) {
		const uint64_t o = base + lane;
		const uint32_t w = o < o_end ? mask[o] : 0u;

		if (ballot64(w != 0) == 0) {
			continue;	/* no doc of any pair's set among these ordinals */
		}
		for (uint32_t g = 0; g < ng; g++) {
			const uint64_t b = ballot64(((w >> g) & 1u) && o >= s_from[g]);

			if (lane == g) {
				c += (uint32_t)__popcll(b);
			}
		}
	}
	if (lane < ng) {
		run_cnt[(size_t)lane * ((size_t)n_runs + 1) + r] = c;
	}
}

__global__ void __launch_bounds__(MD_THREADS)
k_md_scan(uint32_t *run_cnt, uint32_t n_runs, uint32_t limit, uint32_t *counts, uint32_t *more)
{
	__shared__ uint32_t s_w[MD_WAVES];
	const uint32_t g = blockIdx.x;
	const unsigned tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
	uint32_t *row = run_cnt + (size_t)g * ((size_t)n_runs + 1);
	uint32_t carry = 0;	/* the same in every thread */

	for (uint32_t base = 0; base < n_runs; base += MD_THREADS) {
		const uint32_t i = base + tid;
		const uint32_t v = i < n_runs ? row[i] : 0u;
		uint32_t x = v, pre = 0, tot = 0;

		/* inclusive scan of the wavefront, then the wavefronts' sums */
		for (unsigned d = 1; d < WAVE; d <<= 1) {
			const uint32_t y = (uint32_t)__shfl_up((int)x, d);

			if (lane >= d) {
				x += y;
			}
		}
		if (lane == WAVE - 1) {
			s_w[wid] = x;
		}
		__syncthreads();
		for (unsigned w = 0; w < MD_WAVES; w++) {
			pre += w < wid ? s_w[w] : 0u;
			tot += s_w[w];
		}
		if (i < n_runs) {
			row[i] = carry + pre + x - v;
		}
		carry += tot;
		__syncthreads();
	}
	if (tid == 0) {
		row[n_runs] = carry;
		counts[g] = min(carry, limit);
		more[g] = carry > limit;
	}
}

/* run_cnt: after k_md_scan, cell (g, r) = the rank of run r's first match, cell (g, n_runs) = the row's sum */
__global__ void __launch_bounds__(MD_THREADS)
k_md_emit(const uint32_t *__restrict__ mask, const uint64_t *__restrict__ doc_ids, uint64_t n_docs, uint32_t run,
    uint32_t n_runs, const uint32_t *__restrict__ from_ord, uint32_t ng, const uint32_t *__restrict__ run_cnt,
    uint32_t limit, uint32_t cap, uint64_t *ids)
{
	__shared__ uint32_t s_from[MD_GROUP_MAX];
	const unsigned tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;

	if (tid < MD_GROUP_MAX) {
		s_from[tid] = tid < ng ? from_ord[tid] : 0xffffffffu;
	}
	__syncthreads();
	const uint64_t r = (uint64_t)blockIdx.x * MD_WAVES + wid;

	if (r >= n_runs) {
		return;
	}
	uint32_t mybase = 0xffffffffu;	/* lane g: the rank of pair g's next match */
	bool act = false;

	if (lane < ng) {
		const uint32_t *row = run_cnt + (size_t)lane * ((size_t)n_runs + 1);

		mybase = row[r];
		act = mybase < limit && row[r + 1] > mybase;
	}
	if (ballot64(act) == 0) {
		return;		/* beyond every page, or nothing of any pair in this run */
	}
	const uint64_t o_beg = r * run, o_end = min(o_beg + run, n_docs);
	const uint64_t below = (1ull << lane) - 1;

	for (uint64_t base = o_beg; base < o_end; base += WAVE) {
		uint64_t rest = ballot64(act && mybase < limit);	/* the pairs whose page is not full yet */

		if (rest == 0) {
			break;
		}
		const uint64_t o = base + lane;
		const uint32_t w = o < o_end ? mask[o] : 0u;

		if (ballot64(w != 0) == 0) {
			continue;
		}
		while (rest) {
			const unsigned g = (unsigned)__builtin_ctzll(rest);

			rest &= rest - 1;
			const bool hit = ((w >> g) & 1u) && o >= s_from[g];
			const uint64_t b = ballot64(hit);

			if (b == 0) {
				continue;
			}
			const uint32_t rank = (uint32_t)__shfl((int)mybase, (int)g) + (uint32_t)__popcll(b & below);

			if (hit && rank < limit && rank < cap) {
				ids[(size_t)g * cap + rank] = doc_ids[o];
			}
			if (lane == g) {
				mybase += (uint32_t)__popcll(b);
			}
		}
	}
}

/* ------------------------------------------------------------------ */

void
md_free(nxsgpu_index_t *ix)
{
	if (ix->md) {
		side_close(&ix->md->side, true);
		delete ix->md;
		ix->md = NULL;
	}
}

/* what a pass uploads (q | tok | prog | items | from) and the small block it brings back (counts | more | totals);
 * from_ord stays on the device.  The same layout in the staging area and on the device */
struct md_layout_t {
	count_q_t *	q;
	uint64_t *	tok;
	uint8_t *	prog;
	count_item_t *	items;
	uint64_t *	from;
	size_t		up_len;
	uint32_t	*counts, *more, *totals, *from_ord;
	size_t		out_off, out_len, len;
};

static md_layout_t
md_layout(uint8_t *base, uint32_t G, uint64_t items)
{
	md_layout_t L;
	uint8_t *p = base;

	L.q = carve<count_q_t>(p, G);
	L.tok = carve<uint64_t>(p, (size_t)G * 2 * NXSGPU_MAX_TOKENS);
	L.prog = carve<uint8_t>(p, (size_t)G * NXSGPU_MAX_PROG);
	L.items = carve<count_item_t>(p, items);
	L.from = carve<uint64_t>(p, G);
	L.up_len = (size_t)(p - base);
	L.counts = carve<uint32_t>(p, G);
	L.out_off = (size_t)((uint8_t *)L.counts - base);
	L.more = carve<uint32_t>(p, G);
	L.totals = carve<uint32_t>(p, G);
	L.out_len = (size_t)(p - base) - L.out_off;
	L.from_ord = carve<uint32_t>(p, G);
	L.len = (size_t)(p - base);
	return L;
}

/* the posting range of a plan's token (beyond the snapshot's terms: no postings yet, like count_prepare) */
static inline void
md_tok_range(const nxsgpu_index_t *ix, uint32_t tid, uint64_t *pb, uint64_t *pe)
{
	*pb = tid > ix->n_terms ? 0 : ix->h_post_off[tid];
	*pe = tid > ix->n_terms ? 0 : ix->h_post_off[(size_t)tid + 1];
}

/* a distinct (plan, cursor) pair: the first query that named it, whose row of `ids` receives the page */
struct md_pair_t {
	uint32_t	i;
	uint64_t	from;
};

/* the cross-check route for the distinct pairs */
static int
md_host(nxsgpu_index_t *ix, const nxsgpu_query_t *plans, const std::vector<md_pair_t> &up, uint32_t limit, uint32_t cap,
    uint64_t *ids, uint32_t *u_counts, uint32_t *u_more, uint32_t *u_totals)
{
	const uint64_t P = ix->n_post, D = ix->n_docs;
	std::vector<uint64_t> h_dt(P), h_ids(D);
	std::vector<uint32_t> pres(D), in((D + 31) / 32);
	hipStream_t st = ix->md->side.st;

	if ((P && hipMemcpyAsync(h_dt.data(), ix->d_post_dt, P * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (D && hipMemcpyAsync(h_ids.data(), ix->d_doc_ids, D * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("match_docs: copying the index back failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	for (size_t u = 0; u < up.size(); u++) {
		const nxsgpu_query_t &q = plans[up[u].i];
		uint64_t n = 0;
		bool more = false;

		std::fill(pres.begin(), pres.end(), 0u);
		std::fill(in.begin(), in.end(), 0u);
		for (uint32_t j = 0; j < q.n_tokens; j++) {
			uint64_t pb, pe;

			md_tok_range(ix, q.term_id[j], &pb, &pe);
			for (uint64_t p = pb; p < pe; p++) {
				const uint64_t d = h_dt[p] >> 32;

				if (d < D) {
					pres[d] |= 1u << j;
				}
			}
		}
		for (uint64_t d = 0; d < D; d++) {
			if (pres[d] != 0 && nxs_ds_eval(q.prog, q.prog_len, pres[d])) {
				in[d >> 5] |= 1u << (d & 31);
				n++;
			}
		}
		u_counts[u] = (uint32_t)nxs_md_page(in.data(), h_ids.data(), D, up[u].from, limit, ids + (size_t)up[u].i * cap,
		    &more);
		u_more[u] = more;
		u_totals[u] = (uint32_t)n;
		ix->md->prof[3] += u_counts[u];
	}
	ix->md->prof[1] += up.size();
	return 0;
}

extern "C" int
nxsgpu_match_docs(nxsgpu_index_t *ix, int algo, const nxsgpu_query_t *plans, uint32_t n, const uint64_t *from,
    uint32_t limit, uint64_t *ids, uint32_t *counts, uint8_t *more, uint32_t *totals)
{
	if (algo != NXSGPU_BM25 && algo != NXSGPU_TF_IDF) {
		set_error("nxsgpu_match_docs: unknown ranking function %d", algo);
		return -1;
	}
	if (limit < 1 || limit > NXSGPU_MATCH_MAX) {
		set_error("nxsgpu_match_docs: limit is 1..%u", NXSGPU_MATCH_MAX);
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	if (n > (1u << 24)) {
		set_error("nxsgpu_match_docs: too many queries");
		return -1;
	}
	memset(counts, 0, (size_t)n * 4);
	memset(more, 0, (size_t)n);
	memset(totals, 0, (size_t)n * 4);

	const uint32_t T = ix->n_terms;
	const uint64_t D = ix->n_docs;
	const bool valid = (algo == NXSGPU_BM25) ? ix->bm25_valid : ix->tfidf_valid;

	if (ix->h_post_off.size() < (size_t)T + 2 || ix->h_post_off[(size_t)T + 1] > ix->n_post || D > 0xfffffffeull) {
		set_error("nxsgpu_match_docs: inconsistent row offsets");
		return -1;
	}
	const uint32_t cap = (uint32_t)std::min<uint64_t>(limit, D);
	/* the distinct pairs that have work to do, in the order they were first met */
	std::vector<md_pair_t> up;
	std::vector<uint32_t> rep(n, ~0u);
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
		if ((q.n_tokens > 8 || ix->cfg.matchdocs_host) && !nxs_ds_prog_ok(q.prog, q.prog_len, q.n_tokens)) {
			set_error("query %u: a malformed postfix program, or one deeper than 64", i);
			return -1;
		}
		for (uint32_t j = 0; j < q.n_tokens; j++) {
			uint64_t pb, pe;

			if (q.term_id[j] == 0) {
				set_error("query %u: bad term id 0", i);
				return -1;
			}
			md_tok_range(ix, q.term_id[j], &pb, &pe);
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
		std::string key((const char *)&q, sizeof(q));

		key.append((const char *)&from[i], sizeof(from[i]));
		const auto at = seen.emplace(std::move(key), (uint32_t)up.size());
		if (at.second) {
			up.push_back(md_pair_t{ i, from[i] });
		}
		rep[i] = at.first->second;
	}
	const uint32_t nu = (uint32_t)up.size();
	if (nu == 0) {
		return 0;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	if (!ix->md) {
		ix->md = new md_state_t();
	}
	md_state_t *md = ix->md;
	side_t *sd = &md->side;

	if (side_open(ix, sd, "match_docs", MD_EVENTS, true) != 0) {
		return -1;
	}
	hipStream_t st = sd->st;
	const bool prof = ix->profiling && sd->ev_ok;
	std::vector<uint32_t> u_counts(nu, 0), u_more(nu, 0), u_totals(nu, 0);

	md->prof[9] += 1;
	if (ix->cfg.matchdocs_host) {
		if (md_host(ix, plans, up, limit, cap, ids, u_counts.data(), u_more.data(), u_totals.data()) != 0) {
			return -1;
		}
	} else {
		const uint32_t run = std::max<uint32_t>(WAVE, ix->cfg.matchdocs_run / WAVE * WAVE);
		const uint64_t n_runs = (D + run - 1) / run;
		const uint64_t items8 = (D + CNT_TILE8_DOCS - 1) / CNT_TILE8_DOCS, items32 = (D + CNT_TILE32_DOCS - 1) / CNT_TILE32_DOCS;
		const size_t row = al256((size_t)(n_runs + 1) * 4), page = (size_t)cap * 8, masks = al256((size_t)D * 4);
		const uint64_t ws = ix->cfg.matchdocs_ws;
		const uint32_t G = (uint32_t)std::min<uint64_t>(std::min(MD_GROUP_MAX, nu),
		    std::max<uint64_t>(1, (ws > masks ? ws - masks : 0) / (row + page)));

		if ((uint64_t)G * items32 > 0x7fffffffull || n_runs > 0x7fffffffull) {
			set_error("match_docs plan too large");
			return -1;
		}
		const md_layout_t L0 = md_layout(NULL, G, (uint64_t)G * items32);
		const size_t o_mask = al256(L0.len), o_cnt = o_mask + masks, o_ids = o_cnt + al256((size_t)G * row);
		const size_t ws_need = o_ids + (size_t)G * page + 512;

		if (side_room(sd, "match_docs", L0.len + 512, ws_need) != 0) {
			return -1;
		}
		uint8_t *h = (uint8_t *)(((uintptr_t)sd->pin + 255) & ~(uintptr_t)255);
		uint8_t *d = (uint8_t *)(((uintptr_t)sd->ws + 255) & ~(uintptr_t)255);
		uint32_t *d_mask = (uint32_t *)(d + o_mask), *d_cnt = (uint32_t *)(d + o_cnt);
		uint64_t *d_ids = (uint64_t *)(d + o_ids);
		const uint32_t run_blocks = (uint32_t)((n_runs + MD_WAVES - 1) / MD_WAVES);

		for (uint32_t u0 = 0; u0 < nu; u0 += G) {
			const uint32_t m = std::min(G, nu - u0);
			const md_layout_t H = md_layout(h, G, (uint64_t)G * items32), Dv = md_layout(d, G, (uint64_t)G * items32);
			uint32_t n_items = 0;

			memset(h, 0, H.up_len);
			for (uint32_t g = 0; g < m; g++) {
				const nxsgpu_query_t &q = plans[up[u0 + g].i];
				count_q_t &c = H.q[g];
				const uint64_t ni = q.n_tokens <= 8 ? items8 : items32;

				c.nt = q.n_tokens;
				c.prog_len = q.prog_len;
				c.out = g;
				c.tok_base = g * 2 * NXSGPU_MAX_TOKENS;
				c.prog_base = g * NXSGPU_MAX_PROG;
				memcpy(c.truth, q.truth, sizeof(c.truth));
				for (uint32_t j = 0; j < q.n_tokens; j++) {
					md_tok_range(ix, q.term_id[j], &H.tok[c.tok_base + 2 * j], &H.tok[c.tok_base + 2 * j + 1]);
				}
				memcpy(H.prog + c.prog_base, q.prog, q.prog_len);
				for (uint64_t r = 0; r < ni; r++) {
					H.items[n_items].q = g;
					H.items[n_items++].r = (uint32_t)r;
				}
				H.from[g] = up[u0 + g].from;
			}
			if (hipMemcpyAsync(d, h, H.up_len, hipMemcpyHostToDevice, st) != hipSuccess ||
			    hipMemsetAsync(d + Dv.out_off, 0, Dv.len - Dv.out_off, st) != hipSuccess ||
			    hipMemsetAsync(d_mask, 0, D * 4, st) != hipSuccess) {
				set_error("match_docs upload failed");
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
			a.totals = Dv.totals;
			a.mask = d_mask;
			if (prof) (void)hipEventRecord(sd->ev[0], st);
			hipLaunchKernelGGL(k_md_mask, dim3(n_items), dim3(CNT_THREADS), 0, st, a);
			if (prof) (void)hipEventRecord(sd->ev[1], st);
			hipLaunchKernelGGL(k_md_from, dim3(1), dim3(WAVE), 0, st, (const uint64_t *)ix->d_doc_ids, D,
			    (const uint64_t *)Dv.from, m, Dv.from_ord);
			if (prof) (void)hipEventRecord(sd->ev[2], st);
			hipLaunchKernelGGL(k_md_count, dim3(run_blocks), dim3(MD_THREADS), 0, st, (const uint32_t *)d_mask, D, run,
			    (uint32_t)n_runs, (const uint32_t *)Dv.from_ord, m, d_cnt);
			if (prof) (void)hipEventRecord(sd->ev[3], st);
			hipLaunchKernelGGL(k_md_scan, dim3(m), dim3(MD_THREADS), 0, st, d_cnt, (uint32_t)n_runs, limit, Dv.counts,
			    Dv.more);
			if (prof) (void)hipEventRecord(sd->ev[4], st);
			hipLaunchKernelGGL(k_md_emit, dim3(run_blocks), dim3(MD_THREADS), 0, st, (const uint32_t *)d_mask,
			    (const uint64_t *)ix->d_doc_ids, D, run, (uint32_t)n_runs, (const uint32_t *)Dv.from_ord, m,
			    (const uint32_t *)d_cnt, limit, cap, d_ids);
			if (prof) (void)hipEventRecord(sd->ev[5], st);
			if (hipGetLastError() != hipSuccess) {
				set_error("match_docs kernel launch failed");
				(void)hipStreamSynchronize(st);
				return -1;
			}
			if (hipMemcpyAsync(h + H.out_off, d + Dv.out_off, H.out_len, hipMemcpyDeviceToHost, st) != hipSuccess ||
			    hipStreamSynchronize(st) != hipSuccess) {
				set_error("match_docs pass failed: %s", hipGetErrorString(hipGetLastError()));
				return -1;
			}
			/* the pages: counts[g] ids per pair, into the row of the first query that named the pair */
			for (uint32_t g = 0; g < m; g++) {
				const uint32_t c = std::min(H.counts[g], cap);

				u_counts[u0 + g] = c;
				u_more[u0 + g] = H.more[g];
				u_totals[u0 + g] = H.totals[g];
				md->prof[3] += c;
				if (c && hipMemcpyAsync(ids + (size_t)up[u0 + g].i * cap, d_ids + (size_t)g * cap, (size_t)c * 8,
				    hipMemcpyDeviceToHost, st) != hipSuccess) {
					set_error("match_docs: copying a page back failed");
					(void)hipStreamSynchronize(st);
					return -1;
				}
			}
			if (hipStreamSynchronize(st) != hipSuccess) {
				set_error("match_docs pass failed: %s", hipGetErrorString(hipGetLastError()));
				return -1;
			}
			if (prof) {
				for (int e = 0; e < 5; e++) {
					md->prof[4 + e] += side_elapsed(sd, e, e + 1);
				}
			}
			md->prof[0] += m;
			md->prof[2] += 1;
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t u = rep[i];

		if (u == ~0u) {
			continue;
		}
		counts[i] = u_counts[u];
		more[i] = u_more[u] != 0;
		totals[i] = u_totals[u];
		if (up[u].i != i && counts[i]) {
			memcpy(ids + (size_t)i * cap, ids + (size_t)up[u].i * cap, (size_t)counts[i] * 8);
		}
	}
	return 0;
}

extern "C" void
nxsgpu_match_docs_profile(nxsgpu_index_t *ix, double out[NXSGPU_MATCHDOCS_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_MATCHDOCS_PROF);
	if (ix->md) {
		memcpy(out, ix->md->prof, sizeof(ix->md->prof));
		if (reset) {
			memset(ix->md->prof, 0, sizeof(ix->md->prof));
		}
	}
}
