/*
 * nxs_gpu_prefix.hip -- prefix completion (nxsgpu_complete): for every prefix the dictionary terms that
 * have a posting in a live doc and begin with its bytes, best k by (df descending, term id ascending), and
 * how many there are.
 *
 * In byte-lexicographic order the terms that begin with p are ONE contiguous range, so nothing is
 * screened and nothing is queued:
 *
 *   the order    a permutation of the BK nodes whose term has df > 0 (the CSR's live posting count), any
 *                length, sorted by their bytes; beside entry i its selection key ~df << 32 | term id.
 *                Built on the device by the first call and again when nxsgpu_index::px_gen has moved:
 *                k_px_live compacts the live nodes, then one stable rocprim::radix_sort_pairs per 8-byte
 *                chunk of the terms, last chunk first (k_px_keys packs chunk c big-endian, zero-padded:
 *                terms hold no NUL byte, so a shorter term sorts before its extensions); the number of
 *                passes follows the longest live term.  k_px_pairs then writes the keys.
 *   k_px_range   per prefix two binary searches: the first entry that is not below p, and the first entry
 *                above every extension of p.  Both compare p against the first len(p) bytes of a term --
 *                no successor string is built (a trailing 0xFF byte has none).  matches = hi - lo, exact.
 *   k_px_select  one WORKGROUP (256 threads) per prefix, k rounds of a group-wide minimum over the range:
 *                round r delivers the smallest key above round r - 1's (the keys are distinct).  The round
 *                structure is k_sg_select's (nxs_gpu_fuzzy.hip), a sibling rather than a shared kernel:
 *                that one reads 16-byte keys out of per-token segments and is launched per wavefront,
 *                which is right for its segments (nearly all <= 64 matches); a one-byte prefix ranges
 *                over tens of thousands of entries, k x range / 64 dependent loads per lane on a single
 *                wavefront, so the range is spread over four wavefronts here.  (Chosen from that count,
 *                not from a measurement: NOTES.md.)
 *
 * The pass has a side_t of its own (stream, workspace, pinned staging, events: nxs_gpu_int.h): one upload,
 * the two kernels, one copy back; blocking.  Under NXS_GPU_COMPLETE=host every prefix takes the host ranker
 * (nxs_complete.h) over the host dictionary (dict_host_build): the cross-check route.
 */
#include "nxs_gpu_int.h"
#include "nxs_complete.h"

#define	PX_GROUP	256

static __device__ __forceinline__ uint32_t
px_df(const uint64_t *__restrict__ post_off, uint32_t n_terms, uint32_t term)
{
	return (term >= 1 && term <= n_terms) ? (uint32_t)(post_off[term + 1] - post_off[term]) : 0;
}

/* the nodes with df > 0, in any order (the sort's keys are distinct: the result does not depend on it);
 * cnt[0] = how many, cnt[1] = the longest of their terms */
__global__ void __launch_bounds__(256)
k_px_live(const nxsgpu_bknode_t *__restrict__ bk, uint32_t n_bk, const uint64_t *__restrict__ post_off,
    uint32_t n_terms, uint32_t *node, uint32_t *cnt)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;

	if (i < n_bk && px_df(post_off, n_terms, bk[i].term_id)) {
		const uint32_t pos = atomicAdd(&cnt[0], 1u);
		if (pos < n_bk) {
			node[pos] = i;
		}
		atomicMax(&cnt[1], (uint32_t)bk[i].str_len);
	}
}

/* bytes [8 c, 8 c + 8) of every entry's term, big-endian, zero beyond the term's end */
__global__ void __launch_bounds__(256)
k_px_keys(const nxsgpu_bknode_t *__restrict__ bk, const uint8_t *__restrict__ bytes,
    const uint32_t *__restrict__ node, uint32_t n, uint32_t chunk, uint64_t *keys)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;

	if (i < n) {
		const nxsgpu_bknode_t nd = bk[node[i]];
		uint64_t key = 0;

		for (uint32_t b = 0; b < 8; b++) {
			const uint32_t at = chunk * 8 + b;
			key = (key << 8) | (at < nd.str_len ? bytes[(size_t)nd.str_off + at] : 0);
		}
		keys[i] = key;
	}
}

/* the selection key beside every entry of the order */
__global__ void __launch_bounds__(256)
k_px_pairs(const nxsgpu_bknode_t *__restrict__ bk, const uint64_t *__restrict__ post_off, uint32_t n_terms,
    const uint32_t *__restrict__ node, uint32_t n, uint64_t *key)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;

	if (i < n) {
		const uint32_t term = bk[node[i]].term_id;
		key[i] = ((uint64_t)(uint32_t)~px_df(post_off, n_terms, term) << 32) | term;
	}
}

/*
 * Where a term stands against prefix p: -1 below p (and not an extension of it: a proper prefix of p
 * included), 0 an extension of p (p itself included), +1 above every extension.  Monotone over the order.
 */
static __device__ __forceinline__ int
px_cmp(const nxsgpu_bknode_t &nd, const uint8_t *__restrict__ bytes, const uint8_t *__restrict__ p, uint32_t plen)
{
	const uint32_t m = min((uint32_t)nd.str_len, plen);

	for (uint32_t j = 0; j < m; j++) {
		const uint8_t a = bytes[(size_t)nd.str_off + j], b = p[j];
		if (a != b) {
			return a < b ? -1 : 1;
		}
	}
	return nd.str_len < plen ? -1 : 0;
}

/* one thread per prefix: range[i] = [lo, hi) of the order, matches[i] = hi - lo */
__global__ void __launch_bounds__(64)
k_px_range(const nxsgpu_bknode_t *__restrict__ bk, const uint8_t *__restrict__ bytes,
    const uint32_t *__restrict__ node, uint32_t n_e, const uint8_t *__restrict__ pbytes,
    const uint32_t *__restrict__ poff, uint32_t n, uint2 *range, uint32_t *matches)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;

	if (i >= n) {
		return;
	}
	const uint8_t *p = pbytes + poff[i];
	const uint32_t plen = poff[i + 1] - poff[i];
	uint32_t a = 0, b = n_e, lo;

	while (a < b) {			/* first entry with cmp >= 0 */
		const uint32_t mid = a + (b - a) / 2;
		if (px_cmp(bk[node[mid]], bytes, p, plen) < 0) {
			a = mid + 1;
		} else {
			b = mid;
		}
	}
	lo = a;
	b = n_e;
	while (a < b) {			/* first entry with cmp > 0 */
		const uint32_t mid = a + (b - a) / 2;
		if (px_cmp(bk[node[mid]], bytes, p, plen) <= 0) {
			a = mid + 1;
		} else {
			b = mid;
		}
	}
	range[i] = make_uint2(lo, a);
	if (matches) {
		matches[i] = a - lo;
	}
}

void
px_launch_range(nxsgpu_index_t *ix, hipStream_t st, const uint8_t *d_bytes, const uint32_t *d_off, uint32_t n,
    uint2 *d_range, uint32_t *d_matches)
{
	const px_state_t *px = ix->px;

	hipLaunchKernelGGL(k_px_range, dim3((n + 63) / 64), dim3(64), 0, st,
	    ix->d_bk, ix->d_bk_bytes, px->d_node, px->n_e, d_bytes, d_off, n, d_range, d_matches);
}

/*
 * One workgroup per prefix: round r delivers the r-th smallest key of the range -- the smallest one above
 * the previous round's (no key is 0: term ids start at 1).  Every thread looks at its stride of the range (its first item stays in a
 * register: ranges of up to PX_GROUP entries are read once), the wavefronts' minima meet in LDS.  Exact
 * for ranges of any length.
 */
__global__ void __launch_bounds__(PX_GROUP)
k_px_select(const uint64_t *__restrict__ key, const uint2 *__restrict__ range, uint32_t k,
    uint32_t *term_ids, uint32_t *df, uint32_t *counts)
{
	__shared__ uint64_t s_w[PX_GROUP / WAVE];
	const uint32_t px = blockIdx.x;
	const unsigned tid = threadIdx.x, wid = tid >> 6;
	const uint2 rg = range[px];
	const uint32_t s = rg.x, n = rg.y - rg.x;
	const uint32_t nout = min(k, n);
	const uint64_t none = ~0ull;
	uint64_t mine = none, prev = 0;

	if (tid < n) {
		mine = key[s + tid];
	}
	for (uint32_t r = 0; r < nout; r++) {
		uint64_t best = none;

		if (tid < n && mine > prev) {
			best = mine;
		}
		for (uint32_t i = tid + PX_GROUP; i < n; i += PX_GROUP) {
			const uint64_t c = key[s + i];
			if (c > prev && c < best) {
				best = c;
			}
		}
		for (int o = 32; o; o >>= 1) {
			const uint64_t c = (uint64_t)__shfl_xor((long long)best, o);
			if (c < best) {
				best = c;
			}
		}
		if ((tid & 63) == 0) {
			s_w[wid] = best;
		}
		__syncthreads();
		best = s_w[0];
		for (unsigned w = 1; w < PX_GROUP / WAVE; w++) {
			if (s_w[w] < best) {
				best = s_w[w];
			}
		}
		__syncthreads();
		if (tid == 0) {
			const uint64_t at = (uint64_t)px * k + r;
			term_ids[at] = (uint32_t)best;
			df[at] = ~(uint32_t)(best >> 32);
		}
		prev = best;
	}
	if (tid == 0) {
		counts[px] = nout;
	}
}

void
px_free(nxsgpu_index_t *ix)
{
	px_state_t *px = ix->px;

	if (!px) {
		return;
	}
	side_close(&px->side, true);
	(void)hipFree(px->d_node);
	(void)hipFree(px->d_key);
	delete px;
	ix->px = NULL;
}

#ifdef NXS_TEST_HOOKS
int
px_test_image(nxsgpu_index_t *ix, uint64_t sc[4], const uint32_t **d_node, const uint64_t **d_key)
{
	const px_state_t *px = ix->px;

	memset(sc, 0, 4 * sizeof(uint64_t));
	*d_node = NULL;
	*d_key = NULL;
	if (!px) {
		return 0;
	}
	if (px->side.st && hipStreamSynchronize(px->side.st) != hipSuccess) {
		set_error("nxsgpu_test_term_image: hipStreamSynchronize failed");
		return -1;
	}
	sc[0] = px->built;
	sc[1] = px->built_gen;
	sc[2] = px->n_e;
	sc[3] = px->builds;
	*d_node = px->d_node;
	*d_key = px->d_key;
	return 0;
}
#endif /* NXS_TEST_HOOKS */

/* the order of the index's current generation, on the device */
static int
px_build_order(nxsgpu_index_t *ix)
{
	px_state_t *px = ix->px;
	const uint32_t n = ix->n_bk;
	const double t0 = now_ms();
	uint32_t *d_node[2] = { NULL, NULL }, *d_cnt = NULL, h_cnt[2] = { 0, 0 };
	uint64_t *d_keys[2] = { NULL, NULL };
	void *d_tmp = NULL;
	size_t tmp_bytes = 0;
	uint32_t n_e = 0, chunks = 0;
	unsigned grid = 0;
	int cur = 0, ret = -1;

	(void)hipFree(px->d_node);
	(void)hipFree(px->d_key);
	px->d_node = NULL;
	px->d_key = NULL;
	px->n_e = 0;
	px->built = false;
	if (n) {
		HIP_TRY(hipMalloc(&d_node[0], (size_t)n * 4));
		HIP_TRY(hipMalloc(&d_cnt, 8));
		HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, px->side.st));
		hipLaunchKernelGGL(k_px_live, dim3((n + 255) / 256), dim3(256), 0, px->side.st,
		    ix->d_bk, n, ix->d_post_off, ix->n_terms, d_node[0], d_cnt);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, 8, hipMemcpyDeviceToHost, px->side.st));
		HIP_TRY(hipStreamSynchronize(px->side.st));
	}
	n_e = std::min(h_cnt[0], n);
	if (n_e) {
		chunks = std::max<uint32_t>(1, (h_cnt[1] + 7) / 8);
		grid = (n_e + 255) / 256;
		HIP_TRY(hipMalloc(&d_node[1], (size_t)n_e * 4));
		HIP_TRY(hipMalloc(&d_keys[0], (size_t)n_e * 8));
		HIP_TRY(hipMalloc(&d_keys[1], (size_t)n_e * 8));
		HIP_TRY(rocprim::radix_sort_pairs(NULL, tmp_bytes, d_keys[0], d_keys[1], d_node[0], d_node[1],
		    (size_t)n_e, 0, 64, px->side.st));
		HIP_TRY(hipMalloc(&d_tmp, tmp_bytes ? tmp_bytes : 8));
		/* LSD over the chunks: the sort is stable, so after the pass on chunk c the entries are in order
		 * of their bytes from 8 c on */
		for (uint32_t c = chunks; c-- > 0; ) {
			hipLaunchKernelGGL(k_px_keys, dim3(grid), dim3(256), 0, px->side.st,
			    ix->d_bk, ix->d_bk_bytes, d_node[cur], n_e, c, d_keys[0]);
			HIP_TRY(hipGetLastError());
			HIP_TRY(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_keys[0], d_keys[1], d_node[cur], d_node[cur ^ 1],
			    (size_t)n_e, 0, 64, px->side.st));
			cur ^= 1;
		}
		/* (d_keys[0] becomes the selection keys: it is kept) */
		hipLaunchKernelGGL(k_px_pairs, dim3(grid), dim3(256), 0, px->side.st,
		    ix->d_bk, ix->d_post_off, ix->n_terms, d_node[cur], n_e, d_keys[0]);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(px->side.st));
		px->d_node = d_node[cur];
		px->d_key = d_keys[0];
		d_node[cur] = NULL;
		d_keys[0] = NULL;
	}
	px->n_e = n_e;
	px->built = true;
	px->built_gen = ix->px_gen;
	px->prof[4] = now_ms() - t0;
	px->prof[5] = n_e;
	px->prof[7] += 1;
	px->builds++;
	ret = 0;
fail:
	if (ret != 0) {
		(void)hipStreamSynchronize(px->side.st);
	}
	(void)hipFree(d_node[0]);
	(void)hipFree(d_node[1]);
	(void)hipFree(d_keys[0]);
	(void)hipFree(d_keys[1]);
	(void)hipFree(d_cnt);
	(void)hipFree(d_tmp);
	return ret;
}

/* the host rankers' dictionary of the index's current generation */
static int
px_build_host(nxsgpu_index_t *ix)
{
	px_state_t *px = ix->px;
	const double t0 = now_ms();

	px->h_built = false;
	if (dict_host_build(ix, px->side.st, &px->dict, "complete") != 0) {
		return -1;
	}
	px->h_built = true;
	px->h_gen = ix->px_gen;
	px->prof[4] = now_ms() - t0;
	px->prof[5] = (double)px->dict.h_terms.size();
	px->prof[7] += 1;
	px->builds++;
	return 0;
}

/* the state, and the order (host: the host copy) of the index's current generation */
int
px_prepare(nxsgpu_index_t *ix, bool host)
{
	if (!ix->px) {
		ix->px = new px_state_t();
	}
	px_state_t *px = ix->px;

	if (side_open(ix, &px->side, "complete", 3, true) != 0) {
		return -1;
	}
	if (host) {
		return px->h_built && px->h_gen == ix->px_gen ? 0 : px_build_host(ix);
	}
	return px->built && px->built_gen == ix->px_gen ? 0 : px_build_order(ix);
}

/* one device pass over all n prefixes: one upload from pinned memory, the kernels, one copy back; blocking */
static int
px_pass(nxsgpu_index_t *ix, const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t k,
    uint32_t *o_ids, uint32_t *o_df, uint32_t *o_counts, uint32_t *o_matches)
{
	px_state_t *px = ix->px;
	side_t *sd = &px->side;
	const uint32_t blen = off[n] - off[0];
	/* up: offsets | bytes; down: the term-list block */
	const size_t up_bytes = (((size_t)n + 1) * 4 + blen + 16 + 15) & ~(size_t)15;
	const size_t dn_bytes = tl_bytes(n, k);
	hipStream_t st = sd->st;
	const bool prof = ix->profiling && sd->ev_ok;

	if (side_room(sd, "complete", up_bytes + dn_bytes, up_bytes + dn_bytes + (size_t)n * sizeof(uint2) + 4 * 256) != 0) {
		return -1;
	}
	uint32_t *const h_off = (uint32_t *)sd->pin;
	uint8_t *const h_dn = sd->pin + up_bytes;
	uint8_t *p = (uint8_t *)sd->ws;
	uint8_t *d_up = carve<uint8_t>(p, up_bytes);
	uint8_t *d_dn = carve<uint8_t>(p, dn_bytes);
	uint2 *d_range = carve<uint2>(p, n);
	uint32_t *d_off = (uint32_t *)d_up;
	uint8_t *d_bytes = d_up + ((size_t)n + 1) * 4;
	const tl_block_t d = tl_layout(d_dn, n, k);

	for (uint32_t i = 0; i <= n; i++) {
		h_off[i] = off[i] - off[0];
	}
	memcpy(sd->pin + ((size_t)n + 1) * 4, bytes + off[0], blen);
	if (hipMemcpyAsync(d_up, sd->pin, up_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
	    hipMemsetAsync(d_dn, 0, dn_bytes, st) != hipSuccess) {
		set_error("complete upload failed");
		return -1;
	}
	if (prof) (void)hipEventRecord(sd->ev[0], st);
	px_launch_range(ix, st, d_bytes, d_off, n, d_range, d.matches);
	if (prof) (void)hipEventRecord(sd->ev[1], st);
	hipLaunchKernelGGL(k_px_select, dim3(n), dim3(PX_GROUP), 0, st, px->d_key, d_range, k, d.ids, d.df, d.counts);
	if (prof) (void)hipEventRecord(sd->ev[2], st);
	if (hipGetLastError() != hipSuccess) {
		set_error("complete kernel launch failed");
		(void)hipStreamSynchronize(st);
		return -1;
	}
	if (hipMemcpyAsync(h_dn, d_dn, dn_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("complete pass failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	if (prof) {
		px->prof[0] += 1;
		px->prof[1] += side_elapsed(sd, 0, 2);
		px->prof[2] += side_elapsed(sd, 0, 1);
		px->prof[3] += side_elapsed(sd, 1, 2);
	}
	tl_copy_out(h_dn, n, k, o_ids, o_df, o_counts, o_matches);
	return 0;
}

extern "C" int
nxsgpu_complete(nxsgpu_index_t *ix, const uint8_t *bytes, const uint32_t *off, uint32_t n, uint32_t k,
    uint32_t *term_ids, uint32_t *df, uint32_t *counts, uint32_t *matches)
{
	const int go = tl_enter(ix, "nxsgpu_complete", "prefixes", k, NXS_COMPLETE_MAX, off, n, term_ids, df, counts, matches);

	if (go != 0) {
		return go < 0 ? -1 : 0;
	}
	if (px_prepare(ix, ix->cfg.complete_host) != 0) {
		return -1;
	}
	px_state_t *px = ix->px;

	if (ix->cfg.complete_host) {
		const dict_host_t &dc = px->dict;

		for (uint32_t i = 0; i < n; i++) {
			nxs_complete_rank(dc.h_terms.data(), dc.h_lens.data(), dc.h_dfs.data(), dc.h_ids.data(),
			    dc.h_terms.size(), bytes + off[i], off[i + 1] - off[i], k, term_ids + (size_t)i * k,
			    df + (size_t)i * k, &counts[i], &matches[i]);
		}
		px->prof[6] += n;
		return 0;
	}
	if (!px->n_e) {
		return 0;
	}
	return px_pass(ix, bytes, off, n, k, term_ids, df, counts, matches);
}

extern "C" void
nxsgpu_complete_profile(nxsgpu_index_t *ix, double out[NXSGPU_COMPLETE_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_COMPLETE_PROF);
	if (ix->px) {
		memcpy(out, ix->px->prof, sizeof(ix->px->prof));
		if (reset) {
			memset(ix->px->prof, 0, sizeof(ix->px->prof));
		}
	}
}
