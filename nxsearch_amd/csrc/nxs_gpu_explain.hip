/*
 * nxs_gpu_explain.hip -- explanations (nxsgpu_explain): for every returned doc of every query, what each
 * token of the query's token list added to its score -- the reference's float of that (term, doc) and the
 * term count -- or that the doc does not hold the term.  run_query_logic (search.c:236-270) adds exactly
 * these floats, in token order, so the present cells of a row summed in f32 in ascending token order are the
 * row's score, bit for bit.
 *
 * The pass is post-hoc: it reads final doc ids and the index (the primary CSR d_post_dt for the lookup and
 * the tf, d_post[algo] for the float at the same position -- the REGULAR posting of a TF-IDF dense term
 * keeps the uncapped float, k_impacts_csr; its outlier list lies behind cap_post and is never looked at),
 * and no scan, replay or count kernel knows of it.
 *
 *   k_explain    one workgroup (a wavefront) per (query, block of 64 results); a lane owns one result.  The
 *                lane finds its doc's ordinal (nxs_ex_ordinal over d_doc_ids), then the token loop runs
 *                wave-uniform: the token's list bounds and bitmap row are read from the uploaded token table
 *                by all lanes at the same address, the lookup is nxs_ex_find (nxs_explain.h): the doc's
 *                block bit first where the term has a bitmap row, a branch-free lower bound else.  The 64
 *                lanes probe the same top levels of the same list.  Cells are written with plain stores,
 *                row-major (result, token); present cells are counted per wavefront (one atomic each).
 *                The lane's work is ex_lane(), host + device, so the same code can be run over host arrays.
 *
 * The pass has a side_t of its own (stream, grow-only workspace, pinned staging, events: nxs_gpu_int.h): it runs beside batches and fuzzy passes in flight, takes none of their slots, and is
 * blocking.  It is cut into chunks of at most cfg.explain_rows cells (NXS_GPU_EXPLAIN_ROWS; a chunk holds
 * whole result rows and at least one); a chunk is a contiguous run of the caller's results, so what comes
 * back is copied straight into the caller's arrays.  Nothing exists until the first call.
 */
#include "nxs_gpu_int.h"
#include "nxs_explain.h"

/* one token of one query: its list in the CSR and its bitmap row (~0: none) */
struct ex_tok_t {
	uint64_t	beg, end;
	uint32_t	row, pad;
};

/* one workgroup: results [res0, res0 + n_res) of the chunk, tokens [tok0, tok0 + n_tok) of the table,
 * cells from cell0 (chunk-relative) */
struct ex_blk_t {
	uint32_t	res0, n_res, tok0, n_tok;
	uint64_t	cell0;
};

struct ex_state_t {
	side_t		side;
	double		prof[NXSGPU_EXPLAIN_PROF];
};

/*
 * One lane's work: result `lane` of block b against the block's tokens; -> its present cells.  Host + device:
 * the kernel below is this function per lane, and a host harness can run the same code over host arrays.
 */
__host__ __device__ static inline uint32_t
ex_lane(const ex_blk_t &b, unsigned lane, const ex_tok_t *__restrict__ toks,
    const uint64_t *__restrict__ res_ids, const uint64_t *__restrict__ doc_ids, uint64_t n_docs,
    const uint64_t *__restrict__ post_dt, const posting_t *__restrict__ post,
    const uint64_t *__restrict__ blkmap, const uint32_t *__restrict__ bmrank, uint64_t bm_words,
    uint32_t *__restrict__ out_tf, float *__restrict__ out_imp, uint8_t *__restrict__ found)
{
	const uint64_t ord = nxs_ex_ordinal(doc_ids, n_docs, res_ids[b.res0 + lane]);
	const bool live = ord != NXS_EX_NONE;
	const uint64_t row = b.cell0 + (uint64_t)lane * b.n_tok;
	uint32_t present = 0;

	found[b.res0 + lane] = live;
	for (uint32_t j = 0; j < b.n_tok; j++) {
		const ex_tok_t t = toks[b.tok0 + j];	/* same address in every lane */
		uint32_t tf = 0;
		float imp = 0.0f;

		if (live && t.beg < t.end) {
			const bool bm = t.row != 0xffffffffu;
			const uint64_t p = nxs_ex_find(post_dt, t.beg, t.end,
			    bm ? blkmap + (uint64_t)t.row * bm_words : (const uint64_t *)NULL,
			    bm ? bmrank + (uint64_t)t.row * (bm_words + 1) : (const uint32_t *)NULL, (uint32_t)ord);

			if (p != NXS_EX_NONE) {
				const float s = post[p].imp;
				/* search.c:258: a negative rank() adds nothing */
				if (s >= 0.0f) {
					tf = (uint32_t)post_dt[p];
					imp = s;
				}
			}
		}
		out_tf[row + j] = tf;
		out_imp[row + j] = imp;
		present += tf != 0;
	}
	return present;
}

__global__ void __launch_bounds__(WAVE)
k_explain(const ex_blk_t *__restrict__ blks, const ex_tok_t *__restrict__ toks,
    const uint64_t *__restrict__ res_ids, const uint64_t *__restrict__ doc_ids, uint64_t n_docs,
    const uint64_t *__restrict__ post_dt, const posting_t *__restrict__ post,
    const uint64_t *__restrict__ blkmap, const uint32_t *__restrict__ bmrank, uint64_t bm_words,
    uint32_t *__restrict__ out_tf, float *__restrict__ out_imp, uint8_t *__restrict__ found,
    unsigned long long *__restrict__ n_present)
{
	const ex_blk_t b = blks[blockIdx.x];
	const unsigned lane = threadIdx.x;
	uint32_t present = 0;

	if (lane < b.n_res) {
		present = ex_lane(b, lane, toks, res_ids, doc_ids, n_docs, post_dt, post, blkmap, bmrank, bm_words,
		    out_tf, out_imp, found);
	}
	for (int o = 32; o; o >>= 1) {
		present += (uint32_t)__shfl_xor((int)present, o);
	}
	if (lane == 0 && present) {
		atomicAdd(n_present, (unsigned long long)present);
	}
}

void
ex_free(nxsgpu_index_t *ix)
{
	if (ix->ex) {
		side_close(&ix->ex->side, true);
		delete ix->ex;
		ix->ex = NULL;
	}
}

/*
 * The next chunk: blocks of at most 64 results of one query each, from result r of query q on, whole result rows
 * and at most max_cells cells (at least one row); q and r move past it.  -> its cells.  A chunk is one run of
 * the caller's results, from the r it started at, and of the caller's cells.
 */
static uint64_t
ex_next_chunk(uint32_t n_queries, const uint32_t *tok_off, const uint64_t *res_off, uint64_t max_cells,
    uint32_t &q, uint64_t &r, std::vector<ex_blk_t> &blks)
{
	const uint64_t r_first = r;
	uint64_t c_cells = 0;

	blks.clear();
	while (q < n_queries) {
		const uint32_t nt = tok_off[q + 1] - tok_off[q];
		const uint64_t r_end = res_off[q + 1];

		if (r >= r_end) {
			q++;		/* (res_off is one run: r is the next query's first result) */
			continue;
		}
		uint64_t take = std::min<uint64_t>(r_end - r, WAVE);
		if (nt && c_cells + take * nt > max_cells) {
			take = (max_cells - std::min(max_cells, c_cells)) / nt;
			if (take == 0 && c_cells == 0) {
				take = 1;
			}
			if (take == 0) {
				break;
			}
		}
		ex_blk_t b;
		b.res0 = (uint32_t)(r - r_first);
		b.n_res = (uint32_t)take;
		b.tok0 = tok_off[q] - tok_off[0];
		b.n_tok = nt;
		b.cell0 = c_cells;
		blks.push_back(b);
		c_cells += take * nt;
		r += take;
		if (c_cells >= max_cells || blks.size() >= (1u << 24)) {
			break;
		}
	}
	return c_cells;
}

extern "C" int
nxsgpu_explain(nxsgpu_index_t *ix, int algo, uint32_t n_queries,
    const uint32_t *tok_off, const uint32_t *tok_ids, const uint64_t *res_off, const uint64_t *doc_ids,
    uint32_t *out_tf, float *out_imp, uint8_t *found)
{
	if (algo != NXSGPU_BM25 && algo != NXSGPU_TF_IDF) {
		set_error("nxsgpu_explain: unknown ranking function %d", algo);
		return -1;
	}
	if (n_queries == 0) {
		return 0;
	}
	const uint64_t n_res = res_off[n_queries] - res_off[0];
	const uint32_t n_tok = tok_off[n_queries] - tok_off[0];
	uint64_t cells = 0;

	for (uint32_t q = 0; q < n_queries; q++) {
		cells += (res_off[q + 1] - res_off[q]) * (uint64_t)(tok_off[q + 1] - tok_off[q]);
	}
	memset(found, 0, (size_t)n_res);
	if (cells) {
		memset(out_tf, 0, (size_t)cells * 4);
		memset(out_imp, 0, (size_t)cells * 4);
	}
	if (n_res == 0 || ix->n_docs == 0) {
		return 0;		/* (no live doc: every row is absent) */
	}
	if (!ix->algo_on[algo] || !ix->d_post[algo]) {
		set_error("nxsgpu_explain: the impacts of ranking function %d are not materialised", algo);
		return -1;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	if (!ix->ex) {
		ix->ex = new ex_state_t();
	}
	ex_state_t *ex = ix->ex;
	side_t *sd = &ex->side;

	if (side_open(ix, sd, "explain", 2, true) != 0) {
		return -1;
	}
	hipStream_t st = sd->st;
	const bool prof = ix->profiling && sd->ev_ok;
	const uint64_t max_cells = std::max<uint64_t>(ix->cfg.explain_rows, 1);

	/* the token table: list bounds from the host's copy of the row offsets (an id outside the dictionary
	 * is an empty list), bitmap rows from bm_terms -- both as the index holds them NOW */
	std::vector<ex_tok_t> toks(n_tok);
	for (uint32_t i = 0; i < n_tok; i++) {
		const uint32_t t = tok_ids[tok_off[0] + i];
		ex_tok_t e = { 0, 0, 0xffffffffu, 0 };

		if (t >= 1 && t <= ix->n_terms && (size_t)t + 1 < ix->h_post_off.size()) {
			e.beg = ix->h_post_off[t];
			e.end = ix->h_post_off[(size_t)t + 1];
			if (e.end > ix->n_post || e.beg > e.end) {
				set_error("nxsgpu_explain: inconsistent row offsets of term %u", t);
				return -1;
			}
			if (ix->d_blkmap && ix->d_bmrank) {
				auto it = std::lower_bound(ix->bm_terms.begin(), ix->bm_terms.end(), t);
				if (it != ix->bm_terms.end() && *it == t) {
					e.row = (uint32_t)(it - ix->bm_terms.begin());
				}
			}
		}
		toks[i] = e;
	}

	/* chunks: runs of whole result rows, at most max_cells cells each (at least one row) */
	uint32_t q = 0;
	uint64_t r = res_off[0];		/* next result (caller's index) */
	uint64_t cell_done = 0;
	std::vector<ex_blk_t> blks;

	ex->prof[0] += 1;
	while (q < n_queries) {
		const uint64_t r_first = r;
		const uint64_t c_cells = ex_next_chunk(n_queries, tok_off, res_off, max_cells, q, r, blks);
		if (blks.empty()) {
			break;
		}
		/* a chunk is one run of the caller's results, [r_first, r), and of its cells */
		const uint64_t c_res = r - r_first;
		const size_t up_blk = al256(blks.size() * sizeof(ex_blk_t));
		const size_t up_tok = al256((size_t)n_tok * sizeof(ex_tok_t));
		const size_t up_ids = al256((size_t)c_res * 8);
		const size_t up_len = up_blk + up_tok + up_ids;
		const size_t dn_tf = al256((size_t)c_cells * 4), dn_imp = dn_tf, dn_found = al256((size_t)c_res), dn_cnt = 256;
		const size_t dn_len = dn_tf + dn_imp + dn_found + dn_cnt;

		/* (exact staging: the token table is as long as the CALL's token lists, no chunk budget bounds it) */
		if (side_room(sd, "explain", up_len + dn_len, up_len + dn_len + 256, true) != 0) {
			return -1;
		}
		uint8_t *h = sd->pin, *d = (uint8_t *)(((uintptr_t)sd->ws + 255) & ~(uintptr_t)255);
		memcpy(h, blks.data(), blks.size() * sizeof(ex_blk_t));
		memcpy(h + up_blk, toks.data(), (size_t)n_tok * sizeof(ex_tok_t));
		memcpy(h + up_blk + up_tok, doc_ids + r_first, (size_t)c_res * 8);
		uint8_t *d_dn = d + up_len, *h_dn = h + up_len;

		if (hipMemcpyAsync(d, h, up_len, hipMemcpyHostToDevice, st) != hipSuccess ||
		    hipMemsetAsync(d_dn, 0, dn_len, st) != hipSuccess) {
			set_error("explain upload failed");
			(void)hipStreamSynchronize(st);
			return -1;
		}
		if (prof) (void)hipEventRecord(sd->ev[0], st);
		hipLaunchKernelGGL(k_explain, dim3((unsigned)blks.size()), dim3(WAVE), 0, st,
		    (const ex_blk_t *)d, (const ex_tok_t *)(d + up_blk), (const uint64_t *)(d + up_blk + up_tok),
		    ix->d_doc_ids, ix->n_docs, ix->d_post_dt, ix->d_post[algo], ix->d_blkmap, ix->d_bmrank, ix->bm_words,
		    (uint32_t *)d_dn, (float *)(d_dn + dn_tf), d_dn + dn_tf + dn_imp,
		    (unsigned long long *)(d_dn + dn_tf + dn_imp + dn_found));
		if (prof) (void)hipEventRecord(sd->ev[1], st);
		if (hipGetLastError() != hipSuccess) {
			set_error("explain kernel launch failed");
			(void)hipStreamSynchronize(st);
			return -1;
		}
		if (hipMemcpyAsync(h_dn, d_dn, dn_len, hipMemcpyDeviceToHost, st) != hipSuccess ||
		    hipStreamSynchronize(st) != hipSuccess) {
			set_error("explain pass failed: %s", hipGetErrorString(hipGetLastError()));
			return -1;
		}
		memcpy(out_tf + cell_done, h_dn, (size_t)c_cells * 4);
		memcpy(out_imp + cell_done, h_dn + dn_tf, (size_t)c_cells * 4);
		memcpy(found + (r_first - res_off[0]), h_dn + dn_tf + dn_imp, (size_t)c_res);
		cell_done += c_cells;
		if (prof) {
			ex->prof[1] += side_elapsed(sd, 0, 1);
		}
		ex->prof[2] += (double)c_cells;
		ex->prof[3] += (double)*(const unsigned long long *)(h_dn + dn_tf + dn_imp + dn_found);
		ex->prof[4] += 1;
	}
	if (cell_done != cells) {
		set_error("nxsgpu_explain: %llu of %llu cells were produced", (unsigned long long)cell_done,
		    (unsigned long long)cells);
		return -1;
	}
	return 0;
}

extern "C" void
nxsgpu_explain_profile(nxsgpu_index_t *ix, double out[NXSGPU_EXPLAIN_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_EXPLAIN_PROF);
	if (ix->ex) {
		memcpy(out, ix->ex->prof, sizeof(ix->ex->prof));
		if (reset) {
			memset(ix->ex->prof, 0, sizeof(ix->ex->prof));
		}
	}
}
