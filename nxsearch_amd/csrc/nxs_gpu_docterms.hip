/*
 * nxs_gpu_docterms.hip -- term vectors of docs (nxsgpu_doc_terms): for every doc of a batch the dictionary
 * terms that have a posting in it, a live df >= mindf and an impact w >= 0 under the ranking function, best k
 * by (w descending, term id ascending), and how many there are -- exactly, however many.
 *
 * There is no forward index on the device and none is built: a doc's term vector is the explain lookup
 * (nxs_explain.h) run over the whole dictionary.  The float is d_post[algo] at the posting's position -- the
 * REGULAR posting of a TF-IDF dense term keeps the uncapped float, its outlier list lies behind cap_post and
 * is never looked at --, the tf is d_post_dt's, the df the list's length.
 *
 *   k_dv_ord     a lane per doc id: its ordinal (nxs_ex_ordinal over d_doc_ids), ~0 = not a live doc.  The
 *                host sorts the live ordinals and drops duplicates: a doc asked twice is answered once.
 *   k_dv_scan    the hot kernel.  Grid (parts, chunks), a workgroup is ONE wavefront: a part is a run of
 *                whole 64-term tiles of the term-id range, a chunk at most 64 ordinals (ascending, in LDS).
 *                Per tile a lane reads one term's list bounds and looks up its bitmap row; then the tile's
 *                lists meet the chunk from the shorter side (nxs_docterms.h), every loop wave-uniform:
 *                  by posting   lists shorter than the chunk, no bitmap row: the lane walks its own list,
 *                               one lower bound per posting over the ordinals in LDS;
 *                  by doc       the other lists, one at a time (ballot + ffs), a LANE PER DOC: 64 docs
 *                               probe one list side by side with nxs_ex_find, as k_explain's lanes do --
 *                               or, when the chunk holds fewer docs than the tile has such lists, a lane
 *                               per term and the doc loop uniform.
 *                Eligible hits are counted (a register per doc lane, LDS atomics by posting; one global
 *                atomic per doc and workgroup at the end) and feed a running top-k per doc in LDS, sorted
 *                ascending by nxs_dv_key: a hit that does not beat the doc's k-th key is dropped on the
 *                spot, the others are inserted one at a time by the whole wavefront (a ballot gives the
 *                position, the lanes behind it shift).  Keys are distinct, so the lists do not depend on
 *                the order hits arrive in.  At the end the lists go to partial[doc][part][k].
 *   k_dv_merge   one wavefront per doc: k rounds of a wave-wide minimum over the HEADS of its parts' lists (they
 *                are ascending: a cursor per part in LDS); lane r then finds the r-th winner's posting again
 *                (nxs_ex_find) for w, tf and df.
 *
 * Device memory is docs x parts x k keys, never a list of hits; a batch whose partial lists would exceed
 * NXS_GPU_DOCTERMS_WS (64 MiB) is cut into passes of whole chunks.  The pass has a side_t of its own (stream, grow-only
 * workspace, pinned staging, events: nxs_gpu_int.h): beside batches and fuzzy passes in flight, none of their slots; blocking.
 * Nothing exists until the first call.  Under NXS_GPU_DOCTERMS=host the posting arrays are copied back and
 * the same lookups (nxs_dv_term) and a plain sort run on the host: the cross-check route.
 */
#include "nxs_gpu_int.h"
#include "nxs_docterms.h"

#define	DV_NONE		(~0ull)
#define	DV_EVENTS	6

struct dv_state_t {
	side_t		side;
	double		prof[NXSGPU_DOCTERMS_PROF];
};

/* the bitmap row of term t, or ~0: a search of the ascending ids of the terms that have one */
static __host__ __device__ __forceinline__ uint32_t
dv_bm_row(const uint32_t *__restrict__ bm_terms, uint32_t n_bm, uint32_t t)
{
	uint32_t base = 0, n = n_bm;

	if (n == 0) {
		return ~0u;
	}
	while (n > 1) {
		const uint32_t half = n >> 1;
		base = bm_terms[base + half - 1] < t ? base + half : base;
		n -= half;
	}
	return bm_terms[base] == t ? base : ~0u;
}

__global__ void
k_dv_ord(const uint64_t *__restrict__ ids, uint32_t n, const uint64_t *__restrict__ doc_ids, uint64_t n_docs,
    uint64_t *__restrict__ ords)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;

	if (i < n) {
		ords[i] = nxs_ex_ordinal(doc_ids, n_docs, ids[i]);
	}
}

/*
 * The pending hits of the wavefront -- lane: (slot j, key) -- into the slots' lists, one at a time.  top: LDS,
 * [slot][k] ascending, padded with ~0.  Called by all 64 lanes.
 */
static __device__ __forceinline__ void
dv_insert_hits(uint64_t *top, uint32_t k, bool hit, uint32_t j, uint64_t key, unsigned lane)
{
	unsigned long long pend = __ballot(hit && key < top[(size_t)j * k + k - 1]);

	while (pend) {
		const int src = __ffsll(pend) - 1;
		const uint32_t jj = (uint32_t)__shfl((int)j, src);
		const uint64_t x = (uint64_t)__shfl((long long)key, src);
		uint64_t *list = top + (size_t)jj * k;

		pend &= pend - 1;
		/* (an earlier hit of this round may have raised the slot's bar) */
		if (x < list[k - 1]) {
			const uint64_t mine = lane < k ? list[lane] : DV_NONE;
			const uint32_t at = (uint32_t)__popcll(__ballot(lane < k && mine < x));

			if (lane >= at && lane + 1 < k) {
				list[lane + 1] = mine;
			}
			if (lane == 0) {
				list[at] = x;
			}
		}
		__syncthreads();	/* (one wavefront: orders the list's stores before the next reads) */
	}
}

__global__ void __launch_bounds__(WAVE)
k_dv_scan(const uint64_t *__restrict__ post_off, const uint64_t *__restrict__ post_dt,
    const posting_t *__restrict__ post, const uint64_t *__restrict__ blkmap, const uint32_t *__restrict__ bmrank,
    uint64_t bm_words, const uint32_t *__restrict__ bm_terms, uint32_t n_bm, uint64_t bm_mindf, uint32_t n_terms,
    const uint32_t *__restrict__ ords, uint32_t n_ords, uint32_t np, uint32_t k, uint32_t mindf,
    uint64_t *__restrict__ partial, uint32_t *matches)
{
	extern __shared__ uint64_t s_top[];		/* [NXS_DV_CHUNK][k] */
	__shared__ uint32_t s_ord[NXS_DV_CHUNK];
	__shared__ uint32_t s_cnt[NXS_DV_CHUNK];
	const uint32_t part = blockIdx.x, d0 = blockIdx.y * NXS_DV_CHUNK;
	const unsigned lane = threadIdx.x;
	const uint32_t nd = min((uint32_t)NXS_DV_CHUNK, n_ords - d0);
	const uint32_t tiles = (n_terms + WAVE - 1) / WAVE;
	const uint32_t t0 = (uint32_t)((uint64_t)part * tiles / np), t1 = (uint32_t)((uint64_t)(part + 1) * tiles / np);
	uint32_t mycnt = 0;

	s_ord[lane] = lane < nd ? ords[d0 + lane] : 0xffffffffu;
	s_cnt[lane] = 0;
	for (uint32_t i = lane; i < NXS_DV_CHUNK * k; i += WAVE) {
		s_top[i] = DV_NONE;
	}
	__syncthreads();
	const uint32_t myord = s_ord[lane];

	for (uint32_t tile = t0; tile < t1; tile++) {
		const uint32_t t = tile * WAVE + lane + 1;
		uint64_t beg = 0, end = 0;
		uint32_t row = ~0u;

		if (t <= n_terms) {
			beg = post_off[t];
			end = post_off[t + 1];
		}
		const uint64_t len = end - beg;
		const bool elig = len > 0 && len >= mindf;

		if (elig && len >= bm_mindf) {
			row = dv_bm_row(bm_terms, n_bm, t);
		}
		const bool shrt = elig && nxs_dv_by_posting(len, nd, row != ~0u);
		unsigned long long lng = __ballot(elig && !shrt);

		/* by posting: the lane walks its own short list */
		for (uint32_t i = 0; __ballot(shrt && i < len); i++) {
			bool hit = false;
			uint32_t j = 0;
			uint64_t key = DV_NONE;

			if (shrt && i < len) {
				j = nxs_dv_slot(s_ord, nd, (uint32_t)(post_dt[beg + i] >> 32));
				if (j != NXS_DV_NOSLOT) {
					const float w = post[beg + i].imp;

					if (w >= 0.0f) {
						hit = true;
						key = nxs_dv_key(w, t);
						atomicAdd(&s_cnt[j], 1u);
					}
				}
				j = hit ? j : 0;
			}
			dv_insert_hits(s_top, k, hit, j, key, lane);
		}
		if (nd < (uint32_t)__popcll(lng)) {
			/* by doc, a lane per term: fewer docs than lists */
			const bool mine = (lng >> lane) & 1;
			const uint64_t *bm = row != ~0u ? blkmap + (uint64_t)row * bm_words : (const uint64_t *)NULL;
			const uint32_t *br = row != ~0u ? bmrank + (uint64_t)row * (bm_words + 1) : (const uint32_t *)NULL;

			for (uint32_t j = 0; j < nd; j++) {
				bool hit = false;
				uint64_t key = DV_NONE;

				if (mine) {
					const uint64_t p = nxs_ex_find(post_dt, beg, end, bm, br, s_ord[j]);

					if (p != NXS_EX_NONE) {
						const float w = post[p].imp;

						if (w >= 0.0f) {
							hit = true;
							key = nxs_dv_key(w, t);
						}
					}
				}
				const uint32_t c = (uint32_t)__popcll(__ballot(hit));
				if (lane == j) {
					mycnt += c;
				}
				dv_insert_hits(s_top, k, hit, j, key, lane);
			}
		} else {
			/* by doc, a lane per doc: the lists one at a time */
			while (lng) {
				const int src = __ffsll(lng) - 1;
				const uint64_t tb = (uint64_t)__shfl((long long)beg, src), te = (uint64_t)__shfl((long long)end, src);
				const uint32_t trow = (uint32_t)__shfl((int)row, src);
				bool hit = false;
				uint64_t key = DV_NONE;

				lng &= lng - 1;
				if (lane < nd) {
					const uint64_t p = nxs_ex_find(post_dt, tb, te,
					    trow != ~0u ? blkmap + (uint64_t)trow * bm_words : (const uint64_t *)NULL,
					    trow != ~0u ? bmrank + (uint64_t)trow * (bm_words + 1) : (const uint32_t *)NULL, myord);

					if (p != NXS_EX_NONE) {
						const float w = post[p].imp;

						if (w >= 0.0f) {
							hit = true;
							key = nxs_dv_key(w, tile * WAVE + (uint32_t)src + 1);
							mycnt++;
						}
					}
				}
				dv_insert_hits(s_top, k, hit, lane, key, lane);
			}
		}
	}
	__syncthreads();
	if (lane < nd) {
		const uint32_t c = s_cnt[lane] + mycnt;

		if (c) {
			atomicAdd(&matches[d0 + lane], c);
		}
	}
	for (uint32_t i = lane; i < nd * k; i += WAVE) {
		const uint32_t j = i / k, r = i - j * k;

		partial[((size_t)(d0 + j) * np + part) * k + r] = s_top[i];
	}
}

#define	DV_PARTS_MAX	4096u		/* NXS_GPU_DOCTERMS_PARTS at most (cfg_from_env) */

/*
 * One wavefront per doc: the k smallest keys of its parts' lists, in order; then w, tf and df of each.  Every
 * part's list is ascending, so a cursor per part (LDS, a byte; lane l owns parts l, l + 64, ... and nobody else
 * touches their cursors) makes a round one load per part -- the heads -- instead of one per kept key.
 */
__global__ void __launch_bounds__(WAVE)
k_dv_merge(const uint64_t *__restrict__ partial, uint32_t np, uint32_t k,
    const uint64_t *__restrict__ post_off, const uint64_t *__restrict__ post_dt, const posting_t *__restrict__ post,
    const uint64_t *__restrict__ blkmap, const uint32_t *__restrict__ bmrank, uint64_t bm_words,
    const uint32_t *__restrict__ bm_terms, uint32_t n_bm, const uint32_t *__restrict__ ords,
    uint32_t *term_ids, float *w, uint32_t *tf, uint32_t *df, uint32_t *counts)
{
	const uint32_t d = blockIdx.x;
	const unsigned lane = threadIdx.x;
	__shared__ uint8_t s_cur[DV_PARTS_MAX];
	const uint64_t *list = partial + (size_t)d * np * k;
	uint64_t won = DV_NONE;
	uint32_t nout = 0;

	for (uint32_t p = lane; p < np; p += WAVE) {
		s_cur[p] = 0;
	}
	for (uint32_t r = 0; r < k; r++) {
		uint64_t mine = DV_NONE, best;
		uint32_t mine_p = 0;

		for (uint32_t p = lane; p < np; p += WAVE) {
			const uint32_t c = s_cur[p];
			const uint64_t head = c < k ? list[(size_t)p * k + c] : DV_NONE;

			if (head < mine) {
				mine = head;
				mine_p = p;
			}
		}
		best = mine;
		for (int o = 32; o; o >>= 1) {
			const uint64_t c = (uint64_t)__shfl_xor((long long)best, o);
			if (c < best) {
				best = c;
			}
		}
		if (best == DV_NONE) {
			break;		/* (every list is used up or padded from here on) */
		}
		if (mine == best) {
			s_cur[mine_p]++;	/* (keys are distinct: one lane) */
		}
		if (lane == r) {
			won = best;
		}
		nout++;
	}
	if (lane < nout) {
		const uint32_t t = (uint32_t)won;
		const uint64_t beg = post_off[t], end = post_off[t + 1];
		const uint32_t row = dv_bm_row(bm_terms, n_bm, t);
		const uint64_t p = nxs_ex_find(post_dt, beg, end,
		    row != ~0u ? blkmap + (uint64_t)row * bm_words : (const uint64_t *)NULL,
		    row != ~0u ? bmrank + (uint64_t)row * (bm_words + 1) : (const uint32_t *)NULL, ords[d]);
		const uint64_t at = (uint64_t)d * k + lane;

		term_ids[at] = t;
		df[at] = (uint32_t)(end - beg);
		if (p != NXS_EX_NONE) {		/* (it is: the key came from this posting) */
			w[at] = post[p].imp;
			tf[at] = (uint32_t)post_dt[p];
		}
	}
	if (lane == 0) {
		counts[d] = nout;
	}
}

void
dv_free(nxsgpu_index_t *ix)
{
	if (ix->dv) {
		side_close(&ix->dv->side, true);
		delete ix->dv;
		ix->dv = NULL;
	}
}

/* the rows of unique doc u (ascending ordinals) into the rows of every caller's doc that has its ordinal */
static void
dv_scatter(const std::vector<uint64_t> &ord_of, const std::vector<uint32_t> &uniq, uint32_t u0, uint32_t m, uint32_t k,
    const uint32_t *s_ids, const float *s_w, const uint32_t *s_tf, const uint32_t *s_df, const uint32_t *s_counts,
    const uint32_t *s_matches, uint32_t *term_ids, float *w, uint32_t *tf, uint32_t *df, uint32_t *counts,
    uint32_t *matches)
{
	for (size_t i = 0; i < ord_of.size(); i++) {
		if (ord_of[i] == NXS_EX_NONE) {
			continue;
		}
		const size_t u = (size_t)(std::lower_bound(uniq.begin(), uniq.end(), (uint32_t)ord_of[i]) - uniq.begin());
		if (u < u0 || u >= (size_t)u0 + m) {
			continue;
		}
		const size_t s = (u - u0) * k, o = i * k;

		memcpy(term_ids + o, s_ids + s, (size_t)k * 4);
		memcpy(w + o, s_w + s, (size_t)k * 4);
		memcpy(tf + o, s_tf + s, (size_t)k * 4);
		memcpy(df + o, s_df + s, (size_t)k * 4);
		counts[i] = s_counts[u - u0];
		matches[i] = s_matches[u - u0];
	}
}

/* the live ordinals of a batch, ascending and distinct */
static void
dv_unique(const std::vector<uint64_t> &ord_of, std::vector<uint32_t> &uniq)
{
	uniq.clear();
	for (uint64_t o : ord_of) {
		if (o != NXS_EX_NONE) {
			uniq.push_back((uint32_t)o);
		}
	}
	std::sort(uniq.begin(), uniq.end());
	uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
}

/*
 * The cross-check route: the posting arrays copied back, nxs_dv_term per term and chunk, a plain sort per doc.
 */
static int
dv_host(nxsgpu_index_t *ix, int algo, const uint64_t *doc_ids, uint32_t n, uint32_t mindf, uint32_t k,
    uint32_t *term_ids, float *w, uint32_t *tf, uint32_t *df, uint32_t *counts, uint32_t *matches, uint8_t *found)
{
	struct hit_t { uint64_t key; float w; uint32_t tf, df; };
	const uint64_t P = ix->n_post, D = ix->n_docs;
	const size_t rows = ix->d_blkmap && ix->d_bmrank ? ix->bm_terms.size() : 0;
	std::vector<uint64_t> h_ids(D), h_dt(P), h_blk(rows * ix->bm_words), ord_of(n);
	std::vector<posting_t> h_post(P);
	std::vector<uint32_t> h_rank(rows * (ix->bm_words + 1)), uniq;
	hipStream_t st = ix->dv->side.st;

	if ((D && hipMemcpyAsync(h_ids.data(), ix->d_doc_ids, D * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (P && hipMemcpyAsync(h_dt.data(), ix->d_post_dt, P * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (P && hipMemcpyAsync(h_post.data(), ix->d_post[algo], P * sizeof(posting_t), hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (rows && ix->bm_words && hipMemcpyAsync(h_blk.data(), ix->d_blkmap, h_blk.size() * 8, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    (rows && hipMemcpyAsync(h_rank.data(), ix->d_bmrank, h_rank.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("doc_terms: copying the index back failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	for (uint32_t i = 0; i < n; i++) {
		ord_of[i] = nxs_ex_ordinal(h_ids.data(), D, doc_ids[i]);
		found[i] = ord_of[i] != NXS_EX_NONE;
	}
	dv_unique(ord_of, uniq);
	const uint32_t nu = (uint32_t)uniq.size();
	std::vector<std::vector<hit_t>> hits(nu);
	std::vector<uint32_t> u_matches(nu, 0), u_counts(nu, 0), u_ids((size_t)nu * k, 0), u_tf((size_t)nu * k, 0), u_df((size_t)nu * k, 0);
	std::vector<float> u_w((size_t)nu * k, 0.0f);
	uint64_t pos[NXS_DV_CHUNK];

	for (uint32_t d0 = 0; d0 < nu; d0 += NXS_DV_CHUNK) {
		const uint32_t nd = std::min<uint32_t>(NXS_DV_CHUNK, nu - d0);

		for (uint32_t t = 1; t <= ix->n_terms; t++) {
			const uint64_t beg = ix->h_post_off[t], end = ix->h_post_off[(size_t)t + 1], len = end - beg;

			if (len == 0 || len < mindf) {
				continue;
			}
			const uint32_t row = dv_bm_row(ix->bm_terms.data(), (uint32_t)rows, t);
			const bool bm = row != ~0u;

			nxs_dv_term(h_dt.data(), beg, end, bm ? h_blk.data() + (size_t)row * ix->bm_words : (const uint64_t *)NULL,
			    bm ? h_rank.data() + (size_t)row * (ix->bm_words + 1) : (const uint32_t *)NULL, uniq.data() + d0, nd,
			    nxs_dv_by_posting(len, nd, bm), pos);
			for (uint32_t j = 0; j < nd; j++) {
				if (pos[j] != NXS_EX_NONE && h_post[pos[j]].imp >= 0.0f) {
					const hit_t h = { nxs_dv_key(h_post[pos[j]].imp, t), h_post[pos[j]].imp, (uint32_t)h_dt[pos[j]], (uint32_t)len };
					hits[d0 + j].push_back(h);
				}
			}
		}
	}
	for (uint32_t u = 0; u < nu; u++) {
		std::sort(hits[u].begin(), hits[u].end(), [](const hit_t &a, const hit_t &b) { return a.key < b.key; });
		u_matches[u] = (uint32_t)hits[u].size();
		u_counts[u] = (uint32_t)std::min<size_t>(k, hits[u].size());
		for (uint32_t r = 0; r < u_counts[u]; r++) {
			u_ids[(size_t)u * k + r] = (uint32_t)hits[u][r].key;
			u_w[(size_t)u * k + r] = hits[u][r].w;
			u_tf[(size_t)u * k + r] = hits[u][r].tf;
			u_df[(size_t)u * k + r] = hits[u][r].df;
		}
	}
	dv_scatter(ord_of, uniq, 0, nu, k, u_ids.data(), u_w.data(), u_tf.data(), u_df.data(), u_counts.data(),
	    u_matches.data(), term_ids, w, tf, df, counts, matches);
	ix->dv->prof[6] += n;
	return 0;
}

extern "C" int
nxsgpu_doc_terms(nxsgpu_index_t *ix, int algo, const uint64_t *doc_ids, uint32_t n, uint32_t mindf, uint32_t k,
    uint32_t *term_ids, float *w, uint32_t *tf, uint32_t *df, uint32_t *counts, uint32_t *matches, uint8_t *found)
{
	if (algo != NXSGPU_BM25 && algo != NXSGPU_TF_IDF) {
		set_error("nxsgpu_doc_terms: unknown ranking function %d", algo);
		return -1;
	}
	if (k < 1 || k > NXSGPU_DOCTERMS_MAX || mindf < 1) {
		set_error("nxsgpu_doc_terms: k is 1..%d, mindf >= 1", NXSGPU_DOCTERMS_MAX);
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	if (n > (1u << 24)) {
		set_error("nxsgpu_doc_terms: too many docs");
		return -1;
	}
	memset(term_ids, 0, (size_t)n * k * 4);
	memset(w, 0, (size_t)n * k * 4);
	memset(tf, 0, (size_t)n * k * 4);
	memset(df, 0, (size_t)n * k * 4);
	memset(counts, 0, (size_t)n * 4);
	memset(matches, 0, (size_t)n * 4);
	memset(found, 0, n);
	if (ix->n_docs == 0) {
		return 0;		/* (no live doc) */
	}
	const uint32_t T = ix->n_terms;
	if (ix->h_post_off.size() < (size_t)T + 2 || ix->h_post_off[(size_t)T + 1] > ix->n_post || ix->n_docs > 0xfffffffeull) {
		set_error("nxsgpu_doc_terms: inconsistent row offsets");
		return -1;
	}
	/* the impacts on demand, as a search does */
	if (ensure_algo(ix, algo) != 0) {
		return -1;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	if (!ix->dv) {
		ix->dv = new dv_state_t();
	}
	dv_state_t *dv = ix->dv;
	side_t *sd = &dv->side;

	if (side_open(ix, sd, "doc_terms", DV_EVENTS, true) != 0) {
		return -1;
	}
	hipStream_t st = sd->st;
	const bool prof = ix->profiling && sd->ev_ok;

	if (ix->cfg.docterms_host) {
		return dv_host(ix, algo, doc_ids, n, mindf, k, term_ids, w, tf, df, counts, matches, found);
	}
	const bool use_bm = ix->d_blkmap && ix->d_bmrank && !ix->bm_terms.empty();
	const uint32_t n_bm = use_bm ? (uint32_t)ix->bm_terms.size() : 0;
	uint64_t bm_mindf = ~0ull;		/* the shortest list that has a row: shorter ones skip the row search */
	for (uint32_t r = 0; r < n_bm; r++) {
		bm_mindf = std::min(bm_mindf, ix->h_post_off[(size_t)ix->bm_terms[r] + 1] - ix->h_post_off[ix->bm_terms[r]]);
	}
	const uint32_t tiles = (T + WAVE - 1) / WAVE;
	const uint32_t np = std::max<uint32_t>(1, std::min(std::min(ix->cfg.docterms_parts, DV_PARTS_MAX), tiles));
	/* docs per pass: whole chunks, the partial lists within the budget (one chunk at least) */
	const uint64_t per_doc = (uint64_t)np * k * 8;
	const uint32_t pass_docs = (uint32_t)std::min<uint64_t>(32768ull * NXS_DV_CHUNK,
	    std::max<uint64_t>(1, ix->cfg.docterms_ws / per_doc / NXS_DV_CHUNK) * NXS_DV_CHUNK);
	const uint32_t pm = std::min(pass_docs, n);	/* unique docs of a pass at most */
	/* workspace: doc ids | ordinals (u64) | bitmap terms | unique ordinals | rows | counts | matches | partial lists */
	const size_t o_ord64 = al256((size_t)n * 8), o_bm = o_ord64 + al256((size_t)n * 8), o_uq = o_bm + al256((size_t)n_bm * 4 + 4);
	const size_t o_dn = o_uq + al256((size_t)n * 4);
	const size_t dn_rows = al256((size_t)pm * k * 4), dn_len = 4 * dn_rows + 2 * al256((size_t)pm * 4);
	const size_t o_part = o_dn + dn_len, ws_need = o_part + (size_t)pm * per_doc + 512;

	if (side_room(sd, "doc_terms", o_part, ws_need) != 0) {
		return -1;
	}
	uint8_t *h = sd->pin, *d = (uint8_t *)(((uintptr_t)sd->ws + 255) & ~(uintptr_t)255);
	std::vector<uint64_t> ord_of(n);
	std::vector<uint32_t> uniq;

	/* ordinals */
	memcpy(h, doc_ids, (size_t)n * 8);
	if (n_bm) {
		memcpy(h + o_bm, ix->bm_terms.data(), (size_t)n_bm * 4);
	}
	if (hipMemcpyAsync(d, h, (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
	    (n_bm && hipMemcpyAsync(d + o_bm, h + o_bm, (size_t)n_bm * 4, hipMemcpyHostToDevice, st) != hipSuccess)) {
		set_error("doc_terms upload failed");
		(void)hipStreamSynchronize(st);
		return -1;
	}
	if (prof) (void)hipEventRecord(sd->ev[0], st);
	hipLaunchKernelGGL(k_dv_ord, dim3((n + 255) / 256), dim3(256), 0, st, (const uint64_t *)d, n, ix->d_doc_ids,
	    ix->n_docs, (uint64_t *)(d + o_ord64));
	if (prof) (void)hipEventRecord(sd->ev[1], st);
	if (hipGetLastError() != hipSuccess ||
	    hipMemcpyAsync(h + o_ord64, d + o_ord64, (size_t)n * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("doc_terms ordinal pass failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	memcpy(ord_of.data(), h + o_ord64, (size_t)n * 8);
	for (uint32_t i = 0; i < n; i++) {
		if (ord_of[i] != NXS_EX_NONE && ord_of[i] >= ix->n_docs) {
			set_error("nxsgpu_doc_terms: ordinal out of range");
			return -1;
		}
		found[i] = ord_of[i] != NXS_EX_NONE;
	}
	dv_unique(ord_of, uniq);
	dv->prof[0] += 1;
	if (prof) {
		dv->prof[1] += side_elapsed(sd, 0, 1);
	}
	const uint32_t nu = (uint32_t)uniq.size();
	if (nu == 0 || T == 0) {
		return 0;
	}
	memcpy(h + o_uq, uniq.data(), (size_t)nu * 4);
	if (hipMemcpyAsync(d + o_uq, h + o_uq, (size_t)nu * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
		set_error("doc_terms upload failed");
		(void)hipStreamSynchronize(st);
		return -1;
	}
	const uint32_t *d_bm = (const uint32_t *)(d + o_bm);
	uint8_t *d_dn = d + o_dn, *h_dn = h + o_dn;
	uint32_t *d_ids = (uint32_t *)d_dn, *d_tf = (uint32_t *)(d_dn + 2 * dn_rows), *d_df = (uint32_t *)(d_dn + 3 * dn_rows);
	float *d_w = (float *)(d_dn + dn_rows);
	uint32_t *d_counts = (uint32_t *)(d_dn + 4 * dn_rows), *d_matches = (uint32_t *)(d_dn + 4 * dn_rows + al256((size_t)pm * 4));

	for (uint32_t u0 = 0; u0 < nu; u0 += pass_docs) {
		const uint32_t m = std::min(pass_docs, nu - u0);
		const uint32_t *d_ords = (const uint32_t *)(d + o_uq) + u0;

		if (hipMemsetAsync(d_dn, 0, dn_len, st) != hipSuccess) {
			set_error("doc_terms pass failed");
			(void)hipStreamSynchronize(st);
			return -1;
		}
		if (prof) (void)hipEventRecord(sd->ev[2], st);
		hipLaunchKernelGGL(k_dv_scan, dim3(np, (m + NXS_DV_CHUNK - 1) / NXS_DV_CHUNK), dim3(WAVE),
		    (size_t)NXS_DV_CHUNK * k * 8, st, ix->d_post_off, ix->d_post_dt, ix->d_post[algo], ix->d_blkmap, ix->d_bmrank,
		    ix->bm_words, d_bm, n_bm, bm_mindf, T, d_ords, m, np, k, mindf, (uint64_t *)(d + o_part), d_matches);
		if (prof) (void)hipEventRecord(sd->ev[3], st);
		hipLaunchKernelGGL(k_dv_merge, dim3(m), dim3(WAVE), 0, st, (const uint64_t *)(d + o_part), np, k, ix->d_post_off,
		    ix->d_post_dt, ix->d_post[algo], ix->d_blkmap, ix->d_bmrank, ix->bm_words, d_bm, n_bm, d_ords, d_ids, d_w,
		    d_tf, d_df, d_counts);
		if (prof) (void)hipEventRecord(sd->ev[4], st);
		if (hipGetLastError() != hipSuccess) {
			set_error("doc_terms kernel launch failed");
			(void)hipStreamSynchronize(st);
			return -1;
		}
		if (hipMemcpyAsync(h_dn, d_dn, dn_len, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipStreamSynchronize(st) != hipSuccess) {
			set_error("doc_terms pass failed: %s", hipGetErrorString(hipGetLastError()));
			return -1;
		}
		const uint32_t *s_counts = (const uint32_t *)(h_dn + 4 * dn_rows);
		const uint32_t *s_matches = (const uint32_t *)(h_dn + 4 * dn_rows + al256((size_t)pm * 4));

		dv_scatter(ord_of, uniq, u0, m, k, (const uint32_t *)h_dn, (const float *)(h_dn + dn_rows),
		    (const uint32_t *)(h_dn + 2 * dn_rows), (const uint32_t *)(h_dn + 3 * dn_rows), s_counts, s_matches,
		    term_ids, w, tf, df, counts, matches);
		if (prof) {
			dv->prof[2] += side_elapsed(sd, 2, 3);
			dv->prof[3] += side_elapsed(sd, 3, 4);
		}
		dv->prof[4] += 1;
		dv->prof[5] += m;
		for (uint32_t u = 0; u < m; u++) {
			dv->prof[7] += s_matches[u];
		}
	}
	return 0;
}

extern "C" void
nxsgpu_doc_terms_profile(nxsgpu_index_t *ix, double out[NXSGPU_DOCTERMS_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_DOCTERMS_PROF);
	if (ix->dv) {
		memcpy(out, ix->dv->prof, sizeof(ix->dv->prof));
		if (reset) {
			memset(ix->dv->prof, 0, sizeof(ix->dv->prof));
		}
	}
}
