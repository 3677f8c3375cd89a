/*
 * nxs_gpu_docset.hip -- a search within a caller's doc-id set (nxsgpu_search_docs): for every plan of a batch the
 * results the reference produces when nxs_resp_addresult is reached only for the docs of the plan's set S --
 * the matches of S fed in descending doc id into the capped heap of `limit` entries, then heap_sort, ties where
 * that heap puts them -- and, on request, |R n S|.
 *
 * The scoring is driven from the docs: |S| x tokens lookups (nxs_docset.h on top of nxs_explain.h's searches),
 * no list is streamed.
 *
 *   k_ds_ord     a lane per id of each distinct set of the call: nxs_ex_ordinal over d_doc_ids, a u32 ordinal or
 *                ~0 for an id that is not in the doc table.  A removed doc keeps its ordinal and has no postings:
 *                it matches nothing.
 *   k_ds_score   one wavefront per (query, chunk of NXS_GPU_DOCSET_CHUNK entries of its set).  Rounds of 64 entries,
 *                a lane per doc, from the chunk's HIGHEST entry down; the token loop is wave-uniform (all lanes
 *                probe the same list, neighbouring ordinals share cache lines).  Matches are compacted by a ballot
 *                and a lane prefix count into the chunk's segment of cand_doc / cand_sc: a segment comes out in
 *                descending doc order and segment numbers rise with the doc range -- the feed order k_replay
 *                assumes (groups from last to first, each already descending).  seg_count per segment, one atomic
 *                add per wavefront into the query's total.  No LDS, plain vector stores.
 *   k_replay     the existing exact replay (nxs_launch_replay) with seg_cap = the chunk: the heap across the lanes
 *                up to limit 64, in LDS up to 8000, in global memory with capacity min(limit, |S|) beyond.
 *
 * Every distinct set of a call is resolved once, before the passes (ids up in slices, ordinals kept on the host at 4 B
 * an id); a pass serves a run of whole queries (one at least) whose arrays fit NXS_GPU_DOCSET_WS and uploads the
 * ordinals of the sets its queries use.  The pass has a side_t of its own (stream, grow-only workspace,
 * pinned staging, events): beside batches and fuzzy passes in flight, none of their slots; blocking.  Nothing
 * exists until the first call.  Under NXS_GPU_DOCSET=host the index arrays are copied back, ordinals and
 * nxs_ds_lane run on the host over the copies, and the candidates go through the same device replay: the
 * cross-check route.
 */
#include "nxs_gpu_int.h"
#include "nxs_gpu_dev.h"
#include "nxs_docset.h"

#define	DS_EVENTS	5

static_assert(sizeof(nxs_ds_post_t) == sizeof(posting_t), "nxs_ds_post_t is posting_t as C sees it");

/* one query of a pass */
struct ds_q_t {
	uint32_t	nt, prog_len;
	uint64_t	set_off;	/* its set's first entry in the pass's id / ordinal arrays */
	uint32_t	set_len;
	uint32_t	seg_first;	/* its first segment = its first work item */
	uint32_t	tok0;		/* its first token in the table */
	uint32_t	pad;
	uint32_t	truth[8];
	uint8_t		prog[NXSGPU_MAX_PROG];
};

struct ds_item_t { uint32_t q, c; };

struct ds_state_t {
	side_t		side;
	double		prof[NXSGPU_DOCSET_PROF];
};

__global__ void __launch_bounds__(256)
k_ds_ord(const uint64_t *__restrict__ ids, uint64_t n, const uint64_t *__restrict__ doc_ids, uint64_t n_docs,
    uint32_t *__restrict__ ord)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;

	if (i < n) {
		const uint64_t o = nxs_ex_ordinal(doc_ids, n_docs, ids[i]);

		ord[i] = o == NXS_EX_NONE ? NXS_DS_NONE : (uint32_t)o;
	}
}

__global__ void __launch_bounds__(WAVE)
k_ds_score(const ds_q_t *__restrict__ qs, const ds_item_t *__restrict__ items, const nxs_ds_tok_t *__restrict__ toks,
    const uint32_t *__restrict__ ord, const uint64_t *__restrict__ post_dt, const posting_t *__restrict__ post,
    const uint64_t *__restrict__ blkmap, const uint32_t *__restrict__ bmrank, uint64_t bm_words, uint32_t chunk,
    uint32_t *__restrict__ seg_count, uint32_t *__restrict__ cand_doc, float *__restrict__ cand_sc,
    uint32_t *__restrict__ totals)
{
	const ds_item_t it = items[blockIdx.x];
	const ds_q_t *__restrict__ Q = &qs[it.q];
	const unsigned lane = threadIdx.x;
	const uint32_t len = Q->set_len;
	const uint32_t e0 = it.c * chunk;
	const uint32_t e1 = min(e0 + chunk, len);
	const uint32_t seg = Q->seg_first + it.c;
	const uint64_t base = (uint64_t)seg * chunk;
	const uint32_t *__restrict__ so = ord + Q->set_off;
	uint32_t n = 0;

	/* from the chunk's highest entry down: lane 0 of round 0 holds the largest doc */
	for (uint32_t r = 0; e0 + r < e1; r += WAVE) {
		const uint32_t i = r + lane;
		uint32_t o = NXS_DS_NONE;
		float sc = 0.0f;
		bool hit = false;

		if (i < e1 - e0) {
			o = so[e1 - 1 - i];
		}
		if (o != NXS_DS_NONE) {
			hit = nxs_ds_lane(o, Q->nt, toks + Q->tok0, Q->truth, Q->prog, Q->prog_len, post_dt,
			    (const nxs_ds_post_t *)post, blkmap, bmrank, bm_words, &sc);
		}
		const uint64_t b = ballot64(hit);
		if (hit) {
			/* (n + prefix < e1 - e0 <= chunk: inside the segment) */
			const uint64_t at = base + n + (uint32_t)__popcll(b & ((1ull << lane) - 1));

			cand_doc[at] = o;
			cand_sc[at] = sc;
		}
		n += (uint32_t)__popcll(b);
	}
	if (lane == 0) {
		seg_count[seg] = n;
		if (n) {
			atomicAdd(&totals[it.q], n);
		}
	}
}

void
ds_free(nxsgpu_index_t *ix)
{
	if (ix->ds) {
		side_close(&ix->ds->side, true);
		delete ix->ds;
		ix->ds = NULL;
	}
}

/*
 * The arrays of a pass of m queries, n_items segments and n_ent set entries.  dev: the device workspace -- what
 * goes up (q .. ord, one copy), what only the kernels touch, what comes back (out_ids .. tot, one copy); !dev:
 * the pinned staging, the same without the middle.
 */
struct ds_layout_t {
	ds_q_t *	q;
	nxs_ds_tok_t *	toks;
	ds_item_t *	items;
	qmeta_t *	qmeta;
	uint64_t *	heap_off;
	uint64_t *	out_off;
	uint32_t *	ord;
	size_t		up_len;
	uint32_t *	seg_count;
	uint32_t *	cand_doc;
	float *		cand_sc;
	float *		gheap_s;
	uint32_t *	gheap_d;
	uint64_t *	out_ids;
	float *		out_sc;
	uint32_t *	out_cnt;
	uint32_t *	tot;
	size_t		down_off, down_len, len;
};

static ds_layout_t
ds_layout(uint8_t *base, bool dev, uint32_t m, uint64_t n_items, uint64_t n_ent, uint32_t chunk, uint64_t out_cap,
    uint64_t gheap_cap)
{
	ds_layout_t L;
	uint8_t *p = base;

	memset(&L, 0, sizeof(L));
	L.q = carve<ds_q_t>(p, m);
	L.toks = carve<nxs_ds_tok_t>(p, (size_t)m * NXSGPU_MAX_TOKENS);
	L.items = carve<ds_item_t>(p, n_items);
	L.qmeta = carve<qmeta_t>(p, m);
	L.heap_off = carve<uint64_t>(p, (size_t)m + 1);
	L.out_off = carve<uint64_t>(p, (size_t)m + 1);
	L.ord = carve<uint32_t>(p, n_ent);
	L.up_len = (size_t)(p - base);
	if (dev) {
		L.seg_count = carve<uint32_t>(p, n_items);
		L.cand_doc = carve<uint32_t>(p, n_items * chunk);
		L.cand_sc = carve<float>(p, n_items * chunk);
		L.gheap_s = carve<float>(p, gheap_cap);
		L.gheap_d = carve<uint32_t>(p, gheap_cap);
	}
	L.out_ids = carve<uint64_t>(p, out_cap);
	L.down_off = (size_t)((uint8_t *)L.out_ids - base);
	L.out_sc = carve<float>(p, out_cap);
	L.out_cnt = carve<uint32_t>(p, m);
	L.tot = carve<uint32_t>(p, m);
	L.len = (size_t)(p - base);
	L.down_len = L.len - L.down_off;
	return L;
}

/* host copies of the index arrays nxs_ds_lane reads (NXS_GPU_DOCSET=host) */
struct ds_host_t {
	std::vector<uint64_t>	doc_ids, post_dt, blkmap;
	std::vector<posting_t>	post;
	std::vector<uint32_t>	bmrank;
};

static int
ds_host_copy(nxsgpu_index_t *ix, int algo, hipStream_t st, ds_host_t &H)
{
	const uint64_t D = ix->n_docs, P = ix->n_post;
	const size_t rows = (ix->d_blkmap && ix->d_bmrank) ? ix->bm_terms.size() : 0;

	H.doc_ids.resize(D);
	H.post_dt.resize(P);
	H.post.resize(P);
	H.blkmap.resize(rows * ix->bm_words);
	H.bmrank.resize(rows * (ix->bm_words + 1));
	if ((D && hipMemcpyAsync(H.doc_ids.data(), ix->d_doc_ids, D * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (P && hipMemcpyAsync(H.post_dt.data(), ix->d_post_dt, P * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (P && hipMemcpyAsync(H.post.data(), ix->d_post[algo], P * sizeof(posting_t), hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (H.blkmap.size() && hipMemcpyAsync(H.blkmap.data(), ix->d_blkmap, H.blkmap.size() * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (H.bmrank.size() && hipMemcpyAsync(H.bmrank.data(), ix->d_bmrank, H.bmrank.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("search_docs: copying the index back failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	return 0;
}

/* the passes of a call: counts, totals and work counters into res / totals, the results of the queries in order
 * into r_ids / r_sc.  0 / -1 */
static int
ds_run(nxsgpu_index_t *ix, int algo, uint64_t limit, const nxsgpu_query_t *plans, uint32_t n,
    const uint64_t *const *sets, const uint32_t *set_len, uint32_t n_sets, const uint32_t *set_of,
    nxsgpu_results_t *res, uint32_t *totals, std::vector<uint64_t> &r_ids, std::vector<float> &r_sc)
{
	const uint32_t T = ix->n_terms;
	const uint64_t D = ix->n_docs;
	const bool valid = (algo == NXSGPU_BM25) ? ix->bm25_valid : ix->tfidf_valid;
	const uint32_t chunk = ix->cfg.docset_chunk;
	const uint32_t kcap = (uint32_t)std::min<uint64_t>(limit, NXSGPU_DOCSET_MAX);
	const int heap = limit <= NXSGPU_FAST_K ? HEAP_REG : limit <= REPLAY_LDS_K ? HEAP_LDS : HEAP_GLOBAL;
	std::vector<uint32_t> act;	/* the queries that have work to do, in order */

	if (ix->h_post_off.size() < (size_t)T + 2 || ix->h_post_off[(size_t)T + 1] > ix->n_post || D > 0xfffffffeull) {
		set_error("nxsgpu_search_docs: inconsistent row offsets");
		return -1;
	}
	for (uint32_t i = 0; i < n; i++) {
		const nxsgpu_query_t &q = plans[i];

		if (q.n_tokens > NXSGPU_MAX_TOKENS || q.prog_len > NXSGPU_MAX_PROG || set_of[i] >= n_sets) {
			set_error("query %u exceeds the device limits", i);
			return -1;
		}
		if (q.n_tokens > 8 && !nxs_ds_prog_ok(q.prog, q.prog_len, q.n_tokens)) {
			set_error("query %u: a malformed postfix program, or one deeper than 64", i);
			return -1;
		}
		if (valid && q.n_tokens && D && T && set_len[set_of[i]]) {
			act.push_back(i);
		}
	}
	if (act.empty()) {
		return 0;
	}
	/* the impacts on demand, as a search does */
	if (ensure_algo(ix, algo) != 0) {
		return -1;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	if (!ix->ds) {
		ix->ds = new ds_state_t();
	}
	{
		ds_state_t *ds = ix->ds;
		side_t *sd = &ds->side;
		ds_host_t HC;
		std::vector<int64_t> set_at(n_sets, -1);	/* a set's first entry in the pass at hand */
		std::vector<uint32_t> pass_sets;
		std::vector<uint32_t> h_cnt, h_cdoc, h_tot;
		std::vector<uint64_t> set_base(n_sets, 0);	/* a used set's first entry in all_ord */
		std::vector<uint8_t> used(n_sets, 0);
		std::vector<uint32_t> all_ord;		/* the ordinals of every used set, resolved once */
		uint64_t n_all = 0;
		std::vector<float> h_csc;

		if (side_open(ix, sd, "search_docs", DS_EVENTS, true) != 0) {
			return -1;
		}
		hipStream_t st = sd->st;
		const bool prof = ix->profiling && sd->ev_ok;
		const bool host = ix->cfg.docset_host;

		ds->prof[0] += 1;
		if (host && ds_host_copy(ix, algo, st, HC) != 0) {
			return -1;
		}
		/*
		 * Every distinct set the call uses is resolved ONCE, whatever the passes below make of the batch: the ids
		 * go up back to back in slices the workspace budget bounds (12 B an id), k_ds_ord runs, the ordinals come
		 * back and stay on the host (4 B an id); a pass uploads the ordinals of its sets, not their ids.
		 */
		for (uint32_t a : act) {
			used[set_of[a]] = 1;
		}
		for (uint32_t s = 0; s < n_sets; s++) {
			if (used[s]) {
				set_base[s] = n_all;
				n_all += set_len[s];
				ds->prof[2] += 1;
			}
		}
		ds->prof[3] += (double)n_all;
		all_ord.resize(n_all);
		if (host) {
			for (uint32_t s = 0; s < n_sets; s++) {
				for (uint32_t i = 0; used[s] && i < set_len[s]; i++) {
					const uint64_t o = nxs_ex_ordinal(HC.doc_ids.data(), D, sets[s][i]);

					all_ord[set_base[s] + i] = o == NXS_EX_NONE ? NXS_DS_NONE : (uint32_t)o;
				}
			}
		} else {
			const uint64_t slice = std::min<uint64_t>(n_all, std::max<uint64_t>(4096, ix->cfg.docset_ws / 12));
			const size_t o_ord = al256((size_t)slice * 8);
			uint32_t s = 0;
			uint64_t in_s = 0;		/* the next id to go up: entry in_s of set s */

			if (side_room(sd, "search_docs", o_ord + slice * 4 + 512, o_ord + slice * 4 + 512) != 0) {
				return -1;
			}
			uint8_t *h = (uint8_t *)(((uintptr_t)sd->pin + 255) & ~(uintptr_t)255);
			uint8_t *d = (uint8_t *)(((uintptr_t)sd->ws + 255) & ~(uintptr_t)255);

			for (uint64_t p0 = 0; p0 < n_all; p0 += slice) {
				const uint64_t cnt = std::min(slice, n_all - p0);

				for (uint64_t got = 0; got < cnt;) {
					while (!used[s] || in_s == set_len[s]) {
						s++;
						in_s = 0;
					}
					const uint64_t take = std::min<uint64_t>(cnt - got, set_len[s] - in_s);

					memcpy((uint64_t *)h + got, sets[s] + in_s, (size_t)take * 8);
					got += take;
					in_s += take;
				}
				if (hipMemcpyAsync(d, h, (size_t)cnt * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
					set_error("search_docs upload failed");
					(void)hipStreamSynchronize(st);
					return -1;
				}
				if (prof) (void)hipEventRecord(sd->ev[0], st);
				hipLaunchKernelGGL(k_ds_ord, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (const uint64_t *)d, cnt,
				    (const uint64_t *)ix->d_doc_ids, D, (uint32_t *)(d + o_ord));
				if (prof) (void)hipEventRecord(sd->ev[1], st);
				if (hipGetLastError() != hipSuccess ||
				    hipMemcpyAsync(h + o_ord, d + o_ord, (size_t)cnt * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
				    hipStreamSynchronize(st) != hipSuccess) {
					set_error("search_docs: resolving the sets failed: %s", hipGetErrorString(hipGetLastError()));
					return -1;
				}
				memcpy(all_ord.data() + p0, h + o_ord, (size_t)cnt * 4);
				if (prof) {
					ds->prof[7] += side_elapsed(sd, 0, 1);
				}
			}
		}
		for (size_t a0 = 0; a0 < act.size();) {
			/* the pass: whole queries while their arrays fit the budget, one at least */
			size_t a1 = a0;
			uint64_t n_items = 0, n_ent = 0, out_cap = 0, bytes = 4096;

			for (uint32_t s : pass_sets) {
				set_at[s] = -1;
			}
			pass_sets.clear();
			for (; a1 < act.size(); a1++) {
				const uint32_t s = set_of[act[a1]], len = set_len[s];
				const uint64_t ch = (len + chunk - 1) / chunk, cap = std::min<uint64_t>(kcap, len);
				const uint64_t cost = sizeof(ds_q_t) + NXSGPU_MAX_TOKENS * sizeof(nxs_ds_tok_t) + 1024 +
				    ch * ((uint64_t)chunk * 8 + 4 + sizeof(ds_item_t)) + cap * (12 + (heap == HEAP_GLOBAL ? 8 : 0)) +
				    (set_at[s] < 0 ? (uint64_t)len * 4 : 0);

				if (a1 > a0 && (bytes + cost > ix->cfg.docset_ws || n_items + ch > 0x7fffffffull)) {
					break;
				}
				bytes += cost;
				n_items += ch;
				out_cap += cap;
				if (set_at[s] < 0) {
					set_at[s] = (int64_t)n_ent;
					n_ent += len;
					pass_sets.push_back(s);
				}
			}
			const uint32_t m = (uint32_t)(a1 - a0);
			const uint64_t gheap_cap = heap == HEAP_GLOBAL ? out_cap : 0;
			const ds_layout_t L0 = ds_layout(NULL, false, m, n_items, n_ent, chunk, out_cap, gheap_cap);
			const ds_layout_t L1 = ds_layout(NULL, true, m, n_items, n_ent, chunk, out_cap, gheap_cap);

			if (side_room(sd, "search_docs", L0.len + 512, L1.len + 512) != 0) {
				return -1;
			}
			uint8_t *h = (uint8_t *)(((uintptr_t)sd->pin + 255) & ~(uintptr_t)255);
			uint8_t *d = (uint8_t *)(((uintptr_t)sd->ws + 255) & ~(uintptr_t)255);
			const ds_layout_t H = ds_layout(h, false, m, n_items, n_ent, chunk, out_cap, gheap_cap);
			const ds_layout_t Dv = ds_layout(d, true, m, n_items, n_ent, chunk, out_cap, gheap_cap);
			uint64_t cells = 0, it = 0, oc = 0;

			memset(h, 0, H.up_len);
			for (uint32_t s : pass_sets) {
				memcpy(H.ord + set_at[s], all_ord.data() + set_base[s], (size_t)set_len[s] * 4);
			}
			for (uint32_t g = 0; g < m; g++) {
				const nxsgpu_query_t &q = plans[act[a0 + g]];
				const uint32_t s = set_of[act[a0 + g]], len = set_len[s];
				const uint32_t ch = (len + chunk - 1) / chunk;
				ds_q_t &c = H.q[g];

				c.nt = q.n_tokens;
				c.prog_len = q.prog_len;
				c.set_off = (uint64_t)set_at[s];
				c.set_len = len;
				c.seg_first = (uint32_t)it;
				c.tok0 = g * NXSGPU_MAX_TOKENS;
				memcpy(c.truth, q.truth, sizeof(c.truth));
				memcpy(c.prog, q.prog, q.prog_len);
				/* the token table: list bounds from the host's copy of the row offsets (an id outside the
				 * dictionary is an empty list), bitmap rows from bm_terms -- as the index holds them NOW */
				for (uint32_t j = 0; j < q.n_tokens; j++) {
					const uint32_t t = q.term_id[j];
					nxs_ds_tok_t e = { 0, 0, NXS_DS_NONE, 0 };

					if (t >= 1 && t <= T) {
						e.beg = ix->h_post_off[t];
						e.end = ix->h_post_off[(size_t)t + 1];
						if (e.end > ix->n_post || e.beg > e.end) {
							set_error("nxsgpu_search_docs: inconsistent row offsets of term %u", t);
							return -1;
						}
						if (ix->d_blkmap && ix->d_bmrank) {
							auto bt = std::lower_bound(ix->bm_terms.begin(), ix->bm_terms.end(), t);
							if (bt != ix->bm_terms.end() && *bt == t) {
								e.row = (uint32_t)(bt - ix->bm_terms.begin());
							}
						}
					}
					H.toks[c.tok0 + j] = e;
				}
				for (uint32_t k = 0; k < ch; k++) {
					H.items[it].q = g;
					H.items[it++].c = k;
				}
				H.qmeta[g].seg_first = c.seg_first;
				H.qmeta[g].n_groups = ch;
				H.heap_off[g] = H.out_off[g] = oc;
				oc += std::min<uint64_t>(kcap, len);
				cells += len;
			}
			H.heap_off[m] = H.out_off[m] = oc;
			if (hipMemcpyAsync(d, h, H.up_len, hipMemcpyHostToDevice, st) != hipSuccess ||
			    hipMemsetAsync(d + Dv.down_off, 0, Dv.down_len, st) != hipSuccess) {
				set_error("search_docs upload failed");
				(void)hipStreamSynchronize(st);
				return -1;
			}
			if (prof) (void)hipEventRecord(sd->ev[2], st);
			if (!host) {
				hipLaunchKernelGGL(k_ds_score, dim3((unsigned)n_items), dim3(WAVE), 0, st, (const ds_q_t *)Dv.q,
				    (const ds_item_t *)Dv.items, (const nxs_ds_tok_t *)Dv.toks, (const uint32_t *)Dv.ord,
				    (const uint64_t *)ix->d_post_dt, (const posting_t *)ix->d_post[algo], (const uint64_t *)ix->d_blkmap,
				    (const uint32_t *)ix->d_bmrank, ix->bm_words, chunk, Dv.seg_count, Dv.cand_doc, Dv.cand_sc, Dv.tot);
				ds->prof[4] += (double)cells;
			} else {
				/* the same segments, filled by the host: nxs_ds_lane per (query, entry) */
				h_cnt.assign(n_items, 0);
				h_tot.assign(m, 0);
				h_cdoc.assign(n_items * chunk, 0);
				h_csc.assign(n_items * chunk, 0.0f);
				for (uint64_t w = 0; w < n_items; w++) {
					const ds_q_t &c = H.q[H.items[w].q];
					const uint32_t e0 = H.items[w].c * chunk, e1 = std::min(e0 + chunk, c.set_len);
					uint32_t cnt = 0;

					for (uint32_t e = e1; e > e0; e--) {
						const uint32_t o = H.ord[c.set_off + e - 1];
						float sc;

						if (o != NXS_DS_NONE && nxs_ds_lane(o, c.nt, H.toks + c.tok0, c.truth, c.prog, c.prog_len,
						    HC.post_dt.data(), (const nxs_ds_post_t *)HC.post.data(), HC.blkmap.data(), HC.bmrank.data(),
						    ix->bm_words, &sc)) {
							h_cdoc[w * chunk + cnt] = o;
							h_csc[w * chunk + cnt++] = sc;
						}
					}
					h_cnt[w] = cnt;
					h_tot[H.items[w].q] += cnt;
				}
				if (hipMemcpyAsync(Dv.seg_count, h_cnt.data(), n_items * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
				    hipMemcpyAsync(Dv.cand_doc, h_cdoc.data(), n_items * chunk * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
				    hipMemcpyAsync(Dv.cand_sc, h_csc.data(), n_items * chunk * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
				    hipMemcpyAsync(Dv.tot, h_tot.data(), (size_t)m * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
				    hipStreamSynchronize(st) != hipSuccess) {
					set_error("search_docs: uploading the host route's candidates failed");
					return -1;
				}
				ds->prof[5] += (double)cells;
			}
			if (prof) (void)hipEventRecord(sd->ev[3], st);
			replay_args_t ra;

			memset(&ra, 0, sizeof(ra));
			ra.qmeta = Dv.qmeta;
			ra.seg_cap = chunk;
			ra.seg_count = Dv.seg_count;
			ra.cand_doc = Dv.cand_doc;
			ra.cand_sc = Dv.cand_sc;
			ra.doc_ids = ix->d_doc_ids;
			ra.k = kcap;
			ra.out_ids = Dv.out_ids;
			ra.out_sc = Dv.out_sc;
			ra.out_count = Dv.out_cnt;
			ra.out_off = Dv.out_off;
			if (heap == HEAP_GLOBAL) {
				ra.gheap_s = Dv.gheap_s;
				ra.gheap_d = Dv.gheap_d;
				ra.heap_off = Dv.heap_off;
			}
			nxs_launch_replay(heap, m, heap == HEAP_LDS ? (size_t)kcap * 8 : 0, st, ra);
			if (prof) (void)hipEventRecord(sd->ev[4], st);
			if (hipGetLastError() != hipSuccess) {
				set_error("search_docs kernel launch failed");
				(void)hipStreamSynchronize(st);
				return -1;
			}
			if (hipMemcpyAsync(h + H.down_off, d + Dv.down_off, H.down_len, hipMemcpyDeviceToHost, st) != hipSuccess ||
			    hipStreamSynchronize(st) != hipSuccess) {
				set_error("search_docs pass failed: %s", hipGetErrorString(hipGetLastError()));
				return -1;
			}
			for (uint32_t g = 0; g < m; g++) {
				const uint32_t i = act[a0 + g];
				const uint32_t cnt = H.out_cnt[g];

				if (cnt > H.out_off[g + 1] - H.out_off[g]) {
					set_error("nxsgpu_search_docs: query %u came back with %u results", i, cnt);
					return -1;
				}
				res->counts[i] = cnt;
				r_ids.insert(r_ids.end(), H.out_ids + H.out_off[g], H.out_ids + H.out_off[g] + cnt);
				r_sc.insert(r_sc.end(), H.out_sc + H.out_off[g], H.out_sc + H.out_off[g] + cnt);
				if (totals) {
					totals[i] = H.tot[g];
				}
				ds->prof[6] += H.tot[g];
				res->candidates += H.tot[g];
			}
			if (prof) {
				if (!host) {
					ds->prof[8] += side_elapsed(sd, 2, 3);
				}
				ds->prof[9] += side_elapsed(sd, 3, 4);
			}
			ds->prof[1] += 1;
			a0 = a1;
		}
	}
	return 0;
}

extern "C" int
nxsgpu_search_docs(nxsgpu_index_t *ix, int algo, uint64_t limit, const nxsgpu_query_t *plans, uint32_t n,
    const uint64_t *const *sets, const uint32_t *set_len, uint32_t n_sets, const uint32_t *set_of,
    nxsgpu_results_t *res, uint32_t *totals)
{
	memset(res, 0, sizeof(*res));
	if (algo != NXSGPU_BM25 && algo != NXSGPU_TF_IDF) {
		set_error("nxsgpu_search_docs: unknown ranking function %d", algo);
		return -1;
	}
	if (limit == 0) {
		set_error("nxsgpu_search_docs: limit must be >= 1");
		return -1;
	}
	if (n > (1u << 24)) {
		set_error("nxsgpu_search_docs: too many queries");
		return -1;
	}
	for (uint32_t s = 0; s < n_sets; s++) {
		if (set_len[s] > NXSGPU_DOCSET_MAX) {
			set_error("nxsgpu_search_docs: set %u holds more than %u ids", s, NXSGPU_DOCSET_MAX);
			return -1;
		}
		for (uint32_t i = 1; i < set_len[s]; i++) {
			if (sets[s][i - 1] >= sets[s][i]) {
				set_error("nxsgpu_search_docs: set %u is not ascending and distinct", s);
				return -1;
			}
		}
	}
	res->n_queries = n;
	res->counts = (uint32_t *)calloc((size_t)n + 1, sizeof(uint32_t));
	res->offsets = (uint64_t *)calloc((size_t)n + 1, sizeof(uint64_t));
	if (!res->counts || !res->offsets) {
		set_error("out of memory");
		nxsgpu_results_free(res);
		return -1;
	}
	if (totals && n) {
		memset(totals, 0, (size_t)n * 4);
	}

	std::vector<uint64_t> r_ids;	/* the results of the queries, in order */
	std::vector<float> r_sc;

	if (n && ds_run(ix, algo, limit, plans, n, sets, set_len, n_sets, set_of, res, totals, r_ids, r_sc) != 0) {
		nxsgpu_results_free(res);
		return -1;
	}
	res->doc_ids = (uint64_t *)malloc((r_ids.size() + 1) * sizeof(uint64_t));
	res->scores = (float *)malloc((r_sc.size() + 1) * sizeof(float));
	if (!res->doc_ids || !res->scores) {
		set_error("out of memory");
		nxsgpu_results_free(res);
		return -1;
	}
	if (!r_ids.empty()) {
		memcpy(res->doc_ids, r_ids.data(), r_ids.size() * sizeof(uint64_t));
		memcpy(res->scores, r_sc.data(), r_sc.size() * sizeof(float));
	}
	for (uint32_t i = 0; i < n; i++) {
		res->offsets[i + 1] = res->offsets[i] + res->counts[i];
	}
	return 0;
}

extern "C" void
nxsgpu_search_docs_profile(nxsgpu_index_t *ix, double out[NXSGPU_DOCSET_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_DOCSET_PROF);
	if (ix->ds) {
		memcpy(out, ix->ds->prof, sizeof(ix->ds->prof));
		if (reset) {
			memset(ix->ds->prof, 0, sizeof(ix->ds->prof));
		}
	}
}
