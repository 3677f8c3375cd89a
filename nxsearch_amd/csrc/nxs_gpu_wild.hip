/*
 * nxs_gpu_wild.hip -- wildcard term matching (nxsgpu_wildcard): for every pattern (`*` any run of bytes, `?`
 * one byte; nxs_wild.h) the dictionary terms that have a posting in a live doc and match it, best k by (df
 * descending, term id ascending), and how many there are -- exactly, however many.
 *
 * The pass reads the order nxs_gpu_prefix.hip owns (the live terms in byte order, beside entry i its
 * selection key ~df << 32 | term id; px_prepare builds it for the index's generation) and builds none of
 * its own.  A pattern whose star is not at its end is not a range of that order: it is a SCAN of the range
 * its literal head selects -- of the whole order when it begins with a metacharacter.
 *
 *   range        the literal head (the bytes before the first metacharacter) through k_px_range's two
 *                binary searches (px_launch_range); an empty head selects [0, n_e).
 *   k_wc_match   the hot kernel.  Grid (parts, patterns): a pattern's range is cut into
 *                min(NXS_GPU_WILD_PARTS, tiles) parts of whole 256-entry tiles, one workgroup each.  The
 *                workgroup stages its pattern in LDS once; per tile a lane owns one entry, rejects it on its
 *                length (without a star it must equal the pattern's, with one it must reach the number of
 *                non-star bytes) and runs nxs_wild_match_inl on the node's 8 inline bytes and, beyond them,
 *                the byte pool.  Matches are counted by ballot + popcount into a per-wavefront register, one
 *                atomic add per workgroup at the end.  The matched keys feed a running top-k in LDS
 *                (s_top, ascending, padded with ~0): a tile enters the merge only when some matched key
 *                beats the current k-th (one ballot per wavefront), and the merge is k rounds of a
 *                group-wide minimum over {kept keys} + {the tile's matched keys} -- k_px_select's round
 *                structure.  At the end the k keys go to partial[pattern][part][k].
 *   k_wc_merge   one workgroup per pattern, k rounds of a group-wide minimum over its parts' keys; writes
 *                term ids, df and counts.
 *
 * Exact for any range length and any number of matches: every member of the global top-k is in the top-k
 * of its part, and the keys are distinct, so nothing depends on the order in which workgroups or atomics
 * land.  Device memory is patterns x parts x k keys, never a list of matches: `*a*` may match half a
 * dictionary.  A batch whose partial lists would exceed WC_WS_BUDGET (64 MiB) is cut into chunks of patterns.
 * (The layout -- parts per pattern, 256-entry tiles, a top-k per workgroup instead of per wavefront -- was
 * chosen from counts, not from a measurement: NOTES.md.)
 *
 * The pass runs on the order's stream (the prefix state's side_t::st: a completion and a wildcard pass are both
 * blocking, one after the other) with a grow-only workspace, pinned staging and events of its own (a side_t that
 * borrows that stream): beside batches and fuzzy passes in flight, none of their slots.  Under NXS_GPU_WILDCARD=host every pattern takes the host
 * ranker (nxs_wild_rank) over a host copy of the BK image: the cross-check route.
 */
#include "nxs_gpu_int.h"
#include "nxs_gpu_dev.h"
#include "nxs_wild.h"

#define	WC_GROUP	256
#define	WC_WS_BUDGET	(64ull << 20)	/* bytes of partial lists per chunk of patterns */
#define	WC_CHUNK_MAX	32768u		/* patterns per chunk at most (the grid's y dimension) */

struct wc_pat_t {
	uint32_t	off, len;	/* its bytes in the packed patterns */
	uint32_t	minlen;		/* bytes that are no star */
	uint32_t	star;		/* it holds a star */
};

struct wc_state_t {
	side_t		side;		/* (st is the prefix state's: wc_prepare) */
	double		prof[NXSGPU_WILDCARD_PROF];
};

/* parts of a range of `len` entries: whole tiles, at most `cap` */
static __host__ __device__ __forceinline__ uint32_t
wc_parts(uint32_t len, uint32_t cap)
{
	const uint32_t tiles = (len + WC_GROUP - 1) / WC_GROUP;

	return tiles < cap ? tiles : cap;
}

__global__ void __launch_bounds__(WC_GROUP)
k_wc_match(const nxsgpu_bknode_t *__restrict__ bk, const uint8_t *__restrict__ bytes,
    const uint32_t *__restrict__ node, const uint64_t *__restrict__ key, const uint2 *__restrict__ range,
    const wc_pat_t *__restrict__ pats, const uint8_t *__restrict__ pbytes, uint32_t cap, uint32_t k,
    uint64_t *partial, uint32_t *matches)
{
	__shared__ uint8_t s_pat[NXS_WILD_MAXLEN + 1];
	__shared__ uint64_t s_top[NXS_WILD_MAX];
	__shared__ uint64_t s_w[WC_GROUP / WAVE];
	__shared__ uint32_t s_flag[WC_GROUP / WAVE];
	__shared__ uint32_t s_cnt[WC_GROUP / WAVE];
	const uint32_t part = blockIdx.x, px = blockIdx.y;
	const unsigned tid = threadIdx.x, wid = tid >> 6;
	const uint2 rg = range[px];
	const uint32_t len = rg.y - rg.x;
	const uint32_t tiles = (len + WC_GROUP - 1) / WC_GROUP, np = wc_parts(len, cap);
	const uint64_t none = ~0ull;

	if (part >= np) {
		return;			/* (the whole workgroup: k_wc_merge reads np parts) */
	}
	const wc_pat_t pt = pats[px];
	const uint32_t plen = min(pt.len, (uint32_t)NXS_WILD_MAXLEN);
	const uint32_t t0 = (uint32_t)((uint64_t)part * tiles / np), t1 = (uint32_t)((uint64_t)(part + 1) * tiles / np);
	uint32_t wcnt = 0;

	for (uint32_t i = tid; i < plen; i += WC_GROUP) {
		s_pat[i] = pbytes[pt.off + i];
	}
	if (tid < NXS_WILD_MAX) {
		s_top[tid] = none;
	}
	__syncthreads();
	for (uint32_t tile = t0; tile < t1; tile++) {
		const uint32_t at = tile * WC_GROUP + tid;
		uint64_t mine = none;
		bool hit = false;

		if (at < len) {
			const nxsgpu_bknode_t nd = bk[node[rg.x + at]];
			const uint32_t tl = nd.str_len;

			if (pt.star ? tl >= pt.minlen : tl == plen) {
				uint64_t inl;

				memcpy(&inl, nd.inl, 8);
				hit = nxs_wild_match_inl(inl, NXS_WILD_INL, bytes + (size_t)nd.str_off, tl, s_pat, plen);
			}
			if (hit) {
				mine = key[rg.x + at];
			}
		}
		wcnt += (uint32_t)__popcll(__ballot(hit));
		/* does some matched key of this tile beat the k-th kept one? */
		const unsigned long long beats = __ballot(hit && mine < s_top[k - 1]);
		if ((tid & 63) == 0) {
			s_flag[wid] = beats != 0;
		}
		__syncthreads();
		if (s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3]) {
			group_topk_take<WC_GROUP>(mine, s_top, k, s_w, tid);
		}
		__syncthreads();
	}
	if ((tid & 63) == 0) {
		s_cnt[wid] = wcnt;
	}
	__syncthreads();
	if (tid == 0) {
		const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
		if (total) {
			atomicAdd(&matches[px], total);
		}
	}
	if (tid < k) {
		partial[((size_t)px * cap + part) * k + tid] = s_top[tid];
	}
}

/* one workgroup per pattern: the k smallest keys of its parts' lists, in order */
__global__ void __launch_bounds__(WC_GROUP)
k_wc_merge(const uint64_t *__restrict__ partial, const uint2 *__restrict__ range, uint32_t cap, uint32_t k,
    uint32_t *term_ids, uint32_t *df, uint32_t *counts)
{
	__shared__ uint64_t s_w[WC_GROUP / WAVE];
	const uint32_t px = blockIdx.x;
	const unsigned tid = threadIdx.x;
	const uint2 rg = range[px];
	const uint32_t n = wc_parts(rg.y - rg.x, cap) * k;
	const uint64_t *list = partial + (size_t)px * cap * k;
	const uint32_t nout = group_topk_merge<WC_GROUP>(list, n, k, s_w, tid, [&](uint32_t r, uint64_t best) {
		const uint64_t at = (uint64_t)px * k + r;

		term_ids[at] = (uint32_t)best;
		df[at] = ~(uint32_t)(best >> 32);
	});

	if (tid == 0) {
		counts[px] = nout;
	}
}

void
wc_free(nxsgpu_index_t *ix)
{
	wc_state_t *wc = ix->wc;

	if (!wc) {
		return;
	}
	side_close(&wc->side, false);	/* (waits for the prefix state's stream: px_free destroys it, afterwards) */
	delete wc;
	ix->wc = NULL;
}

static int
wc_prepare(nxsgpu_index_t *ix)
{
	if (!ix->wc) {
		ix->wc = new wc_state_t();
	}
	if (side_open(ix, &ix->wc->side, "wildcard", 4, false) != 0 || px_prepare(ix, ix->cfg.wild_host) != 0) {
		return -1;
	}
	ix->wc->side.st = ix->px->side.st;
	return 0;
}

/* one device pass over n patterns (a chunk): one upload from pinned memory, the kernels, one copy back; blocking */
static int
wc_pass(nxsgpu_index_t *ix, const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t k,
    uint32_t *o_ids, uint32_t *o_df, uint32_t *o_counts, uint32_t *o_matches)
{
	px_state_t *px = ix->px;
	wc_state_t *wc = ix->wc;
	side_t *sd = &wc->side;
	const uint32_t cap = ix->cfg.wild_parts;
	const uint32_t blen = off[n] - off[0];
	/* up: pattern records | head offsets | pattern bytes | head bytes; down: the term-list block */
	const size_t o_hoff = (size_t)n * sizeof(wc_pat_t), o_pb = o_hoff + ((size_t)n + 1) * 4;
	const size_t o_hb = (o_pb + blen + 15) & ~(size_t)15;
	const size_t up_bytes = (o_hb + blen + 16 + 15) & ~(size_t)15;
	const size_t dn_bytes = tl_bytes(n, k);
	hipStream_t st = sd->st;
	const bool prof = ix->profiling && sd->ev_ok;

	if (side_room(sd, "wildcard", up_bytes + dn_bytes,
	    up_bytes + dn_bytes + (size_t)n * sizeof(uint2) + (size_t)n * cap * k * 8 + 4 * 256) != 0) {
		return -1;
	}
	wc_pat_t *const h_pat = (wc_pat_t *)sd->pin;
	uint32_t *const h_hoff = (uint32_t *)(sd->pin + o_hoff);
	uint8_t *const h_pb = sd->pin + o_pb, *const h_hb = sd->pin + o_hb;
	uint8_t *const h_dn = sd->pin + up_bytes;
	uint8_t *p = (uint8_t *)sd->ws;
	uint8_t *d_up = carve<uint8_t>(p, up_bytes);
	uint8_t *d_dn = carve<uint8_t>(p, dn_bytes);
	uint2 *d_range = carve<uint2>(p, n);
	uint64_t *d_partial = carve<uint64_t>(p, (size_t)n * cap * k);
	const tl_block_t d = tl_layout(d_dn, n, k);
	uint32_t hlen = 0;

	memcpy(h_pb, bytes + off[0], blen);
	for (uint32_t i = 0; i < n; i++) {
		const uint8_t *pat = bytes + off[i];
		const uint32_t plen = off[i + 1] - off[i], head = nxs_wild_head(pat, plen);
		uint32_t lit;

		h_pat[i].off = off[i] - off[0];
		h_pat[i].len = plen;
		h_pat[i].star = (uint32_t)nxs_wild_shape(pat, plen, &lit, &h_pat[i].minlen);
		h_hoff[i] = hlen;
		memcpy(h_hb + hlen, pat, head);
		hlen += head;
	}
	h_hoff[n] = hlen;
	if (hipMemcpyAsync(d_up, sd->pin, up_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
	    hipMemsetAsync(d_dn, 0, dn_bytes, st) != hipSuccess) {
		set_error("wildcard upload failed");
		return -1;
	}
	if (prof) (void)hipEventRecord(sd->ev[0], st);
	px_launch_range(ix, st, d_up + o_hb, (const uint32_t *)(d_up + o_hoff), n, d_range, NULL);
	if (prof) (void)hipEventRecord(sd->ev[1], st);
	hipLaunchKernelGGL(k_wc_match, dim3(cap, n), dim3(WC_GROUP), 0, st, ix->d_bk, ix->d_bk_bytes, px->d_node, px->d_key,
	    d_range, (const wc_pat_t *)d_up, d_up + o_pb, cap, k, d_partial, d.matches);
	if (prof) (void)hipEventRecord(sd->ev[2], st);
	hipLaunchKernelGGL(k_wc_merge, dim3(n), dim3(WC_GROUP), 0, st, d_partial, d_range, cap, k, d.ids, d.df, d.counts);
	if (prof) (void)hipEventRecord(sd->ev[3], st);
	if (hipGetLastError() != hipSuccess) {
		set_error("wildcard kernel launch failed");
		(void)hipStreamSynchronize(st);
		return -1;
	}
	if (hipMemcpyAsync(h_dn, d_dn, dn_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("wildcard pass failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	wc->prof[0] += 1;
	wc->prof[8] += n;
	if (prof) {
		wc->prof[1] += side_elapsed(sd, 0, 3);
		for (int e = 0; e < 3; e++) {
			wc->prof[2 + e] += side_elapsed(sd, e, e + 1);
		}
	}
	tl_copy_out(h_dn, n, k, o_ids, o_df, o_counts, o_matches);
	return 0;
}

extern "C" int
nxsgpu_wildcard(nxsgpu_index_t *ix, const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t k,
    uint32_t *term_ids, uint32_t *df, uint32_t *counts, uint32_t *matches)
{
	const int go = tl_enter(ix, "nxsgpu_wildcard", "patterns", k, NXS_WILD_MAX, off, n, term_ids, df, counts, matches);

	if (go != 0) {
		return go < 0 ? -1 : 0;
	}
	for (uint32_t i = 0; i < n; i++) {
		if (off[i + 1] < off[i] || off[i + 1] - off[i] > NXS_WILD_MAXLEN) {
			set_error("nxsgpu_wildcard: pattern %u is longer than %d bytes", i, NXS_WILD_MAXLEN);
			return -1;
		}
	}
	if (wc_prepare(ix) != 0) {
		return -1;
	}
	px_state_t *px = ix->px;
	wc_state_t *wc = ix->wc;

	if (ix->cfg.wild_host) {
		const dict_host_t &dc = px->dict;

		for (uint32_t i = 0; i < n; i++) {
			nxs_wild_rank(dc.h_terms.data(), dc.h_lens.data(), dc.h_dfs.data(), dc.h_ids.data(),
			    dc.h_terms.size(), bytes + off[i], off[i + 1] - off[i], k, term_ids + (size_t)i * k,
			    df + (size_t)i * k, &counts[i], &matches[i]);
		}
		wc->prof[6] += n;
		return 0;
	}
	if (!px->n_e) {
		return 0;
	}
	/* chunks of patterns: the partial lists of one stay within the budget */
	const uint64_t per = (uint64_t)ix->cfg.wild_parts * k * 8;
	const uint32_t chunk = (uint32_t)std::min<uint64_t>(WC_CHUNK_MAX, std::max<uint64_t>(1, WC_WS_BUDGET / per));

	for (uint32_t lo = 0; lo < n; lo += chunk) {
		const uint32_t m = std::min(chunk, n - lo);

		if (wc_pass(ix, bytes, off + lo, m, k, term_ids + (size_t)lo * k, df + (size_t)lo * k, counts + lo,
		    matches + lo) != 0) {
			return -1;
		}
	}
	return 0;
}

extern "C" void
nxsgpu_wildcard_profile(nxsgpu_index_t *ix, double out[NXSGPU_WILDCARD_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_WILDCARD_PROF);
	if (ix->wc) {
		memcpy(out, ix->wc->prof, sizeof(ix->wc->prof));
		if (reset) {
			memset(ix->wc->prof, 0, sizeof(ix->wc->prof));
		}
	}
	if (ix->px) {
		out[5] = ix->cfg.wild_host ? (double)ix->px->dict.h_terms.size() : (double)ix->px->n_e;
		out[7] = (double)ix->px->builds;
	}
}
