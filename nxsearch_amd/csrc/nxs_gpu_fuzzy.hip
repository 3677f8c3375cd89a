/*
 * nxs_gpu_fuzzy.hip -- BK-tree search on the device: match-first search + frontier search; nxsgpu_fuzzy
 * (MI355X / gfx950 query path of nxsearch; see nxs_gpu_int.h for the map of the files)
 */
#include "nxs_gpu_int.h"
#include "nxs_gpu_dev.h"
#include "nxs_lev.h"

/* ------------------------------------------------------------------ */

struct fz_item_t { uint32_t tok, node; };

struct fz_args_t {
	const nxsgpu_bknode_t *	bk;
	const uint8_t *		bk_bytes;
	const uint8_t *		tok_bytes;
	const uint32_t *	tok_off;
	const uint64_t *	peq;		/* [n_tok][256] */
	const fz_item_t *	cur;
	fz_item_t *		next;
	const uint32_t *	cur_count;
	uint32_t *		next_count;
	uint32_t		cap;
	uint32_t *		best;		/* [n_tok] min BFS index of a usable match */
	unsigned long long *	visited;	/* [n_tok] or NULL */
	uint16_t *		dp_rows;	/* scratch for tokens > 64 bytes */
	uint32_t		dp_stride;
	uint32_t *		overflow;
	uint32_t		prune;		/* drop (token, node) pairs that can no longer win */
	unsigned long long *	evals;		/* distance evaluations (profiling) or NULL */
};

/* distance between token `tok` and the node's term */
__device__ static inline int
fz_distance(const fz_args_t &A, uint32_t tok, const nxsgpu_bknode_t &nd, uint64_t slot)
{
	const uint32_t qoff = A.tok_off[tok], m = A.tok_off[tok + 1] - qoff;
	const uint32_t n = nd.str_len;

	if (m == 0) {
		return (int)n;
	}
	if (m <= NXS_MYERS_MAXPAT) {
		/* Myers bit-vector, pattern = query token */
		const uint64_t *peq = A.peq + (uint64_t)tok * 256;
		nxs_myers_t s;
		nxs_myers_init(&s, m);
		/*
		 * Eight term bytes at a time: their Peq words are eight independent
		 * gathers issued together (one L2 round trip), then the dependent
		 * bit-vector steps.  Fetched inside the step loop they cost one round
		 * trip per byte -- the kernel was bound by exactly that latency.  Bytes
		 * past the term's end index a valid table row and are not stepped.
		 */
		uint64_t w;
		memcpy(&w, nd.inl, 8);
		const uint8_t *rest = A.bk_bytes + nd.str_off;
		for (uint32_t i0 = 0; i0 < n; i0 += 8) {
			uint64_t e[8];
			if (i0) {
				/* (the byte pool carries 16 bytes of slack behind its end) */
				uint32_t lo32, hi32;
				__builtin_memcpy(&lo32, rest + i0, 4);
				__builtin_memcpy(&hi32, rest + i0 + 4, 4);
				w = (uint64_t)lo32 | ((uint64_t)hi32 << 32);
			}
#pragma unroll
			for (int i = 0; i < 8; i++) {
				e[i] = peq[(w >> (8 * i)) & 0xff];
			}
#pragma unroll
			for (int i = 0; i < 8; i++) {
				if (i0 + i < n) {
					nxs_myers_step(&s, e[i]);
				}
			}
		}
		return s.score;
	}
	/* long token: row DP (levdist.c:67-150) in global scratch */
	{
		const uint8_t *a = A.tok_bytes + qoff;		/* length m */
		const uint8_t *b = A.bk_bytes + nd.str_off;	/* length n */
		uint16_t *row = A.dp_rows + slot * A.dp_stride;
		uint32_t la = m, lb = n;
		if (la < lb) {
			const uint8_t *t = a; a = b; b = t;
			const uint32_t tl = la; la = lb; lb = tl;
		}
		if (lb == 0) {
			return (int)la;
		}
		for (uint32_t j = 0; j <= lb; j++) {
			row[j] = (uint16_t)j;
		}
		for (uint32_t i = 0; i < la; i++) {
			uint32_t diag = i, above;
			row[0] = (uint16_t)(i + 1);
			for (uint32_t j = 1; j <= lb; j++) {
				above = row[j];
				uint32_t v = diag + (a[i] != b[j - 1]);
				v = min(v, (uint32_t)row[j - 1] + 1);
				v = min(v, above + 1);
				row[j] = (uint16_t)v;
				diag = above;
			}
		}
		return (int)row[lb];
	}
}

template <bool LONG>
__global__ void
k_bk_level(const fz_args_t A)
{
	__shared__ uint32_t s_wtot[16], s_base;
	const unsigned lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
	const uint32_t count = min(*A.cur_count, A.cap);
	const uint32_t nthreads = gridDim.x * blockDim.x;
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t rounds = (count + nthreads - 1) / nthreads;
	uint32_t n_eval = 0;

	for (uint32_t r = 0; r < rounds; r++) {
		const uint32_t i = r * nthreads + tid;
		uint32_t nkids = 0, first = 0, tok = 0;
		uint64_t bm = 0, full = 0;

		if (i < count) {
			const fz_item_t it = A.cur[i];
			const uint32_t m = A.tok_off[it.tok + 1] - A.tok_off[it.tok];
			tok = it.tok;
			/*
			 * Exact pruning.  The answer is the match of LOWEST BFS rank
			 * (idxterm.c:238-242: first pushed with total > 0; Q7), a node's
			 * descendants all have higher ranks than the node itself (BFS
			 * numbering), and best[tok] only ever decreases.  So once a usable
			 * match of rank r is known, a pair whose node has rank > r can
			 * neither be nor lead to the winner: it is dropped without a distance
			 * computation and without children.  Any value read here -- stale or
			 * written by a concurrent lane of this very level -- is the rank of a
			 * real match, hence a valid bound.  (Off when the caller wants the
			 * reference's visit counts.)
			 */
			const bool dead = A.prune && __hip_atomic_load(&A.best[it.tok], __ATOMIC_RELAXED,
			    __HIP_MEMORY_SCOPE_AGENT) < it.node;
			if (!dead && LONG == (m > NXS_MYERS_MAXPAT)) {
				const nxsgpu_bknode_t nd = A.bk[it.node];
				const int d = fz_distance(A, it.tok, nd, tid);
				n_eval++;
				if (A.visited) {
					atomicAdd(&A.visited[it.tok], 1ull);
				}
				/* match: bktree.c:252-254; winner = first pushed with
				 * total > 0 (idxterm.c:238-242) = min BFS index */
				if (d <= 2 && (nd.flags & 1)) {
					atomicMin(&A.best[it.tok], it.node);
				}
				/* children in slots [max(d-2,0), min(d+2,63)):
				 * bktree.c:150-156,260-264 (x86 shift semantics) */
				const unsigned min_d = d > 2 ? (unsigned)d - 2 : 0;
				const unsigned max_d = min((unsigned)d + 2, 63u);
				const uint64_t lo_mask = ~0ull << (min_d & 63);
				const uint64_t hi_mask = ~0ull >> ((64 - max_d) & 63);
				full = nd.bitmap;
				bm = full & lo_mask & hi_mask;
				nkids = __popcll(bm);
				first = nd.first_child;
			}
		}
		/* wave-level inclusive scan of nkids, one atomic per wavefront */
		uint32_t incl = nkids;
		for (int o = 1; o < WAVE; o <<= 1) {
			const uint32_t v = __shfl_up((int)incl, o);
			if (lane >= (unsigned)o) incl += v;
		}
		const uint32_t total = __shfl((int)incl, WAVE - 1);
		/*
		 * One returning atomic per WORKGROUP and round, not per wavefront: a
		 * single counter word takes ~88 M atomics/s (MI355X_MICROARCH.md,
		 * `dequeue`), and with one per 64 candidates that ceiling -- not memory,
		 * not the DP -- was the 5.4 G candidates/s this kernel ran at.  `rounds`
		 * is uniform over the grid, so every wavefront reaches the barriers.
		 */
		s_wtot[wid] = total;		/* (all lanes write the same value) */
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t sum = 0;
			for (unsigned w = 0; w < nw; w++) {
				const uint32_t tw = s_wtot[w];
				s_wtot[w] = sum;
				sum += tw;
			}
			s_base = sum ? atomicAdd(A.next_count, sum) : 0;
		}
		__syncthreads();
		const uint32_t wbase = s_base + s_wtot[wid];
		__syncthreads();		/* s_wtot is rewritten next round */
		uint32_t o = wbase + incl - nkids;
		/* ascending slot order = the order bktree_search pushes children */
		while (bm) {
			const int slot = __ffsll((long long)bm) - 1;
			bm &= bm - 1;
			const uint32_t child = first + __popcll(full & ((1ull << slot) - 1));
			if (o < A.cap) {
				fz_item_t ni;
				ni.tok = tok;
				ni.node = child;
				A.next[o] = ni;
			} else {
				*A.overflow = 1;
			}
			o++;
		}
	}
	if (A.evals) {
		for (int o = 32; o; o >>= 1) {
			n_eval += (uint32_t)__shfl_xor((int)n_eval, o);
		}
		if (lane == 0 && n_eval) {
			atomicAdd(A.evals, (unsigned long long)n_eval);
		}
	}
}

__global__ void
k_bk_seed(fz_item_t *items, uint32_t *count0, uint32_t n_tok, uint32_t *best,
    unsigned long long *visited)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_tok) {
		fz_item_t it;
		it.tok = i;
		it.node = 0;
		items[i] = it;
		best[i] = 0xffffffffu;
		if (visited) {
			visited[i] = 0;
		}
	}
	if (i == 0) {
		*count0 = n_tok;
	}
}

__global__ void
k_bk_peq(const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tok, uint64_t *peq, uint2 *tokf,
    const uint32_t *tok_rank)
{
	const uint32_t tok = blockIdx.x;
	const uint32_t off = tok_off[tok], m = tok_off[tok + 1] - off;
	if (tokf && threadIdx.x == 0) {
		/* what k_fz_filter compares: the token's byte set, at the token's place in
		 * the length-sorted order */
		uint32_t sg = 0;
		for (uint32_t j = 0; j < m; j++) {
			sg |= 1u << (tok_bytes[off + j] & 31);
		}
		tokf[tok_rank[tok]] = make_uint2(sg, tok);
	}
	for (uint32_t c = threadIdx.x; c < 256; c += blockDim.x) {
		uint64_t bits = 0;
		if (m <= NXS_MYERS_MAXPAT) {
			for (uint32_t j = 0; j < m; j++) {
				if (tok_bytes[off + j] == c) {
					bits |= 1ull << j;
				}
			}
		}
		peq[(uint64_t)tok * 256 + c] = bits;
	}
}

__global__ void
k_bk_finish(const nxsgpu_bknode_t *bk, const uint32_t *best, uint32_t n_tok, uint32_t *term_ids)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_tok) {
		const uint32_t b = best[i];
		term_ids[i] = (b == 0xffffffffu) ? 0 : bk[b].term_id;
	}
}

/* ---- match-first fuzzy search ---------------------------------------- */
/*
 * The level-by-level search above spends its time on the frontier: the winner
 * sits 9-12 levels deep and everything above it has to be expanded (65 M pairs
 * for 1024 tokens over a 1M-term tree).  But the winner has a closed form:
 *
 *   the node of LOWEST BFS rank among those that (1) are a match -- distance
 *   <= 2, on-disk total > 0 -- and (2) bktree_search reaches: at EVERY ancestor
 *   a the slot of the path's child lies in [max(d(q,a)-2, 0), min(d(q,a)+2, 63))
 *   (bktree.c:150-156,260-264; Q8: the range is half-open, so a match is not
 *   always reached).
 *
 * (1) needs no tree: all (token, term) pairs are screened with a necessary
 * condition -- |len difference| <= 2 and, on the sets of bytes the strings
 * contain (hashed to 64 bits), at most 2 bytes on either side that the other
 * string lacks: an edit removes at most one such byte per side -- 0.03-0.6 % of
 * the pairs survive on the synthetic vocabulary and take the exact bit-vector
 * distance.  (2) walks the few real matches up to the root.  The three steps
 * are three launches over flat queues; their result is the same min-rank node
 * (tests and bench.py compare against the level-by-level search with and
 * without pruning, and against the oracle).
 */
#define	FZ_NOPARENT	0xffffffffu
#define	FZF_BUF		192		/* survivors a wavefront stages in LDS */
#define	FZ_MAXLEN	(NXS_MYERS_MAXPAT + 2)	/* longest term that can be within 2 of a token */
#define	FZ_NQ		64		/* survivor sub-queues: a single counter word takes ~88 M atomics/s */
#define	FZ_CSTRIDE	16		/* their counters, one per 64 bytes */

/* per node: its parent and the slot it hangs in */
__global__ void __launch_bounds__(256)
k_bk_aux(const nxsgpu_bknode_t *bk, uint32_t n, uint32_t *parent, uint8_t *slot)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) {
		return;
	}
	if (i == 0) {
		parent[0] = FZ_NOPARENT;
		slot[0] = 0;
	}
	uint64_t bm = bk[i].bitmap;
	uint32_t c = bk[i].first_child;
	while (bm) {
		const int sl = __ffsll((long long)bm) - 1;
		bm &= bm - 1;
		parent[c] = i;
		slot[c] = (uint8_t)sl;
		c++;
	}
}

/* per candidate (the nodes that can win, sorted by term length on the host): the
 * set of bytes its term contains, hashed to 32 bits, and the length */
__global__ void __launch_bounds__(256)
k_fz_sigs(const nxsgpu_bknode_t *bk, const uint8_t *bytes, const uint32_t *cand_node, uint32_t n_c,
    uint32_t *sig, uint8_t *len8)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_c) {
		return;
	}
	const nxsgpu_bknode_t nd = bk[cand_node[i]];
	const uint8_t *str = bytes + nd.str_off;
	uint32_t sg = 0;
	for (uint32_t j = 0; j < nd.str_len; j++) {
		sg |= 1u << (str[j] & 31);
	}
	sig[i] = sg;
	len8[i] = (uint8_t)nd.str_len;
}

/*
 * Screen.  lane = one candidate node (sorted by length: a workgroup's 256 terms
 * span lengths [Lmin, Lmax]), loop = the tokens of length Lmin-2 .. Lmax+2
 * (tokens sorted by length too; their features are wave-uniform and come
 * through the scalar unit, four tokens per round).  grid.y slices the token
 * range.  A pair that passes wrongly (|length difference| = 3 across a length
 * boundary of the workgroup, hash collisions) is dropped by the exact distance.
 */
__global__ void __launch_bounds__(256)
k_fz_filter(const uint32_t *__restrict__ sig, const uint32_t *__restrict__ cand_node,
    const uint8_t *__restrict__ len8, uint32_t n_c, const uint2 *__restrict__ tokf,
    const uint32_t *__restrict__ tok_len_off, fz_item_t *out, uint32_t *out_count, uint32_t qcap,
    uint32_t *overflow)
{
	__shared__ fz_item_t s_buf[4][FZF_BUF];
	/* this workgroup's sub-queue: [sq * qcap, (sq + 1) * qcap) */
	const uint32_t sq = (blockIdx.x + 5 * blockIdx.y) & (FZ_NQ - 1);
	fz_item_t *const sq_out = out + (uint64_t)sq * qcap;
	uint32_t *const sq_count = out_count + sq * FZ_CSTRIDE;
	const unsigned lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const uint32_t first = blockIdx.x * 256, i = first + threadIdx.x;
	const bool valid = i < n_c;
	const uint32_t ts = valid ? sig[i] : 0, nts = ~ts;
	const uint32_t node = valid ? cand_node[i] : 0;
	const uint64_t vmask = ballot64(valid);
	const uint32_t lmin = len8[first], lmax = len8[min(first + 255, n_c - 1)];
	const uint32_t ta = tok_len_off[lmin > 2 ? lmin - 2 : 0];
	const uint32_t tb = tok_len_off[min(lmax + 2, (uint32_t)NXS_MYERS_MAXPAT) + 1];
	const uint32_t per = (tb - ta + gridDim.y - 1) / gridDim.y;
	const uint32_t t0 = ta + blockIdx.y * per, t1 = min(tb, t0 + per);
	uint32_t nb = 0;

	auto flush = [&]() {
		uint32_t base = 0;
		if (lane == 0) {
			base = atomicAdd(sq_count, nb);
		}
		base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
		WAVE_SYNC();
		for (uint32_t e = lane; e < nb; e += WAVE) {
			if (base + e < qcap) {
				sq_out[base + e] = s_buf[wid][e];
			} else {
				*overflow = 1;
			}
		}
		WAVE_SYNC();
		nb = 0;
	};
	auto check = [&](const uint2 f, bool in_range) {
		/* bytes only the term has / only the token has: an edit removes at
		 * most one of each */
		const uint32_t a = __popc(ts & ~f.x), b = __popc(nts & f.x);
		const uint64_t m = in_range ? (ballot64(max(a, b) <= 2u) & vmask) : 0ull;
		if (m) {
			if (lane_of(m)) {
				fz_item_t it;
				it.tok = f.y;
				it.node = node;
				s_buf[wid][nb + lanes_below(m)] = it;
			}
			nb += __popcll(m);
			if (nb > FZF_BUF - WAVE) {
				flush();
			}
		}
	};
	for (uint32_t j = t0; j < t1; j += 4) {
		/* (the array carries four entries of slack behind its end) */
		const uint2 f0 = tokf[j], f1 = tokf[j + 1], f2 = tokf[j + 2], f3 = tokf[j + 3];
		check(f0, true);
		check(f1, j + 1 < t1);
		check(f2, j + 2 < t1);
		check(f3, j + 3 < t1);
	}
	if (nb) {
		flush();
	}
}

/*
 * Exact distance of the screened pairs (grid.y = sub-queue).  A match at
 * distance <= 1 is always reached: every node of a child's subtree is at the
 * child's slot distance s from the ancestor a (slot-63 subtrees, which no search
 * ever enters, are not candidates), so |d(q,a) - s| <= 1 and s lies inside
 * [d(q,a)-2, d(q,a)+2) at every ancestor -- it lowers best[] right here.  A
 * match at distance 2 misses exactly when some ancestor has d(q,a) = s - 2: it
 * goes to the next queue for the walk (one returning atomic per workgroup and
 * round, as in k_bk_level).
 */
__global__ void __launch_bounds__(1024)
k_fz_dist(const fz_args_t A, const fz_item_t *cand, const uint32_t *cand_count, uint32_t qcap, fz_item_t *match,
    uint32_t *match_count, uint32_t mcap)
{
	__shared__ uint32_t s_wtot[16], s_base;
	const unsigned lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
	const uint32_t count = min(cand_count[blockIdx.y * FZ_CSTRIDE], qcap);
	const uint32_t nthreads = gridDim.x * blockDim.x;
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t rounds = (count + nthreads - 1) / nthreads;
	uint32_t n_eval = 0;

	cand += (uint64_t)blockIdx.y * qcap;
	for (uint32_t r = 0; r < rounds; r++) {
		const uint32_t i = r * nthreads + tid;
		fz_item_t it;
		bool hit = false;

		it.tok = it.node = 0;
		if (i < count) {
			it = cand[i];
			const nxsgpu_bknode_t nd = A.bk[it.node];
			const int d = fz_distance(A, it.tok, nd, 0);
			n_eval++;
			if (d <= 1) {
				atomicMin(&A.best[it.tok], it.node);
			} else if (d == 2) {	/* bktree.c:252-254 */
				hit = __hip_atomic_load(&A.best[it.tok], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > it.node;
			}
		}
		const uint64_t m = ballot64(hit);
		s_wtot[wid] = __popcll(m);
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t sum = 0;
			for (unsigned w = 0; w < nw; w++) {
				const uint32_t tw = s_wtot[w];
				s_wtot[w] = sum;
				sum += tw;
			}
			s_base = sum ? atomicAdd(match_count, sum) : 0;
		}
		__syncthreads();
		const uint32_t o = s_base + s_wtot[wid] + lanes_below(m);
		__syncthreads();
		if (hit) {
			if (o < mcap) {
				match[o] = it;
			} else {
				*A.overflow = 1;
			}
		}
	}
	if (A.evals) {
		for (int o = 32; o; o >>= 1) {
			n_eval += (uint32_t)__shfl_xor((int)n_eval, o);
		}
		if (lane == 0 && n_eval) {
			atomicAdd(A.evals, (unsigned long long)n_eval);
		}
	}
}

/* does bktree_search reach the match?  Walk to the root; every ancestor's child
 * range must hold the slot the path leaves it through. */
__global__ void __launch_bounds__(256)
k_fz_chain(const fz_args_t A, const uint32_t *__restrict__ parent, const uint8_t *__restrict__ slot,
    const fz_item_t *match, const uint32_t *match_count, uint32_t mcap)
{
	const unsigned lane = threadIdx.x & 63;
	const uint32_t count = min(*match_count, mcap);
	const uint32_t nthreads = gridDim.x * blockDim.x;
	uint32_t n_eval = 0;

	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nthreads) {
		const fz_item_t it = match[i];
		uint32_t c = it.node;
		bool ok = true;

		for (;;) {
			/* (a match of lower rank is known: this one cannot win -- any value
			 * read is the rank of a reachable match) */
			if (__hip_atomic_load(&A.best[it.tok], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < it.node) {
				ok = false;
				break;
			}
			const uint32_t p = parent[c];
			if (p == FZ_NOPARENT) {
				break;
			}
			const unsigned sl = slot[c];
			const nxsgpu_bknode_t nd = A.bk[p];
			const int d = fz_distance(A, it.tok, nd, 0);
			n_eval++;
			/* bktree.c:150-156,260-264 (x86 shift semantics), as k_bk_level */
			const unsigned min_d = d > 2 ? (unsigned)d - 2 : 0;
			const unsigned max_d = min((unsigned)d + 2, 63u);
			const uint64_t lo_mask = ~0ull << (min_d & 63);
			const uint64_t hi_mask = ~0ull >> ((64 - max_d) & 63);
			if (!(((lo_mask & hi_mask) >> sl) & 1)) {
				ok = false;
				break;
			}
			c = p;
		}
		if (ok) {
			atomicMin(&A.best[it.tok], it.node);
		}
	}
	if (A.evals) {
		for (int o = 32; o; o >>= 1) {
			n_eval += (uint32_t)__shfl_xor((int)n_eval, o);
		}
		if (lane == 0 && n_eval) {
			atomicAdd(A.evals, (unsigned long long)n_eval);
		}
	}
}

/* ------------------------------------------------------------------ */
/* host side of the shim                                               */

void
bk_aux_free(nxsgpu_index_t *ix)
{
	(void)hipFree(ix->d_bk_parent);
	(void)hipFree(ix->d_bk_slot);
	(void)hipFree(ix->d_fz_node);
	(void)hipFree(ix->d_fz_sig);
	(void)hipFree(ix->d_fz_len);
	ix->d_bk_parent = NULL;
	ix->d_bk_slot = NULL;
	ix->d_fz_node = NULL;
	ix->d_fz_sig = NULL;
	ix->d_fz_len = NULL;
	ix->n_fz = 0;
}

/* the match-first search's view of the tree (after d_bk / d_bk_bytes are in place) */
int
bk_aux_build(nxsgpu_index_t *ix, const nxsgpu_bknode_t *nodes, uint32_t n)
{
	bk_aux_free(ix);
	if (n == 0) {
		return 0;
	}
	/* candidates: nodes with postings on disk whose term can be within 2 of a
	 * token of <= 64 bytes; counting sort by length, BFS rank inside a length */
	std::vector<uint32_t> start(FZ_MAXLEN + 2, 0), perm;
	/* (a child in slot 63 is never visited -- the range's upper end is at most 63,
	 * exclusive: bktree.c:150-156 -- and neither is anything below it; BFS
	 * numbering: a parent precedes its children) */
	std::vector<uint8_t> cut(n, 0);
	uint32_t n_c = 0;
	for (uint32_t i = 0; i < n; i++) {
		uint64_t bm = nodes[i].bitmap;
		uint32_t c = nodes[i].first_child;
		while (bm) {
			const int sl = __builtin_ctzll(bm);
			bm &= bm - 1;
			if (c < n) {
				cut[c] = cut[i] | (sl >= 63);
			}
			c++;
		}
	}
	auto is_cand = [&](uint32_t i) { return (nodes[i].flags & 1) && nodes[i].str_len <= FZ_MAXLEN && !cut[i]; };
	for (uint32_t i = 0; i < n; i++) {
		if (is_cand(i)) {
			start[nodes[i].str_len + 1]++;
			n_c++;
		}
	}
	for (uint32_t l = 0; l <= FZ_MAXLEN; l++) {
		start[l + 1] += start[l];
	}
	ix->fz_len_start.assign(start.begin(), start.end());	/* first candidate of every length */
	perm.resize(std::max<uint32_t>(n_c, 1));
	for (uint32_t i = 0; i < n; i++) {
		if (is_cand(i)) {
			perm[start[nodes[i].str_len]++] = i;
		}
	}
	if (hipMalloc(&ix->d_bk_parent, (size_t)n * 4) != hipSuccess ||
	    hipMalloc(&ix->d_bk_slot, (size_t)n + 16) != hipSuccess ||
	    hipMalloc(&ix->d_fz_node, (size_t)std::max<uint32_t>(n_c, 1) * 4) != hipSuccess ||
	    hipMalloc(&ix->d_fz_sig, (size_t)std::max<uint32_t>(n_c, 1) * 4) != hipSuccess ||
	    hipMalloc(&ix->d_fz_len, (size_t)n_c + 16) != hipSuccess ||
	    hipMemcpyAsync(ix->d_fz_node, perm.data(), (size_t)n_c * 4, hipMemcpyHostToDevice, ix->stream_fz) != hipSuccess) {
		bk_aux_free(ix);
		set_error("BK-tree side arrays: out of device memory");
		return -1;
	}
	hipLaunchKernelGGL(k_bk_aux, dim3((n + 255) / 256), dim3(256), 0, ix->stream_fz,
	    ix->d_bk, n, ix->d_bk_parent, ix->d_bk_slot);
	if (n_c) {
		hipLaunchKernelGGL(k_fz_sigs, dim3((n_c + 255) / 256), dim3(256), 0, ix->stream_fz,
		    ix->d_bk, ix->d_bk_bytes, ix->d_fz_node, n_c, ix->d_fz_sig, ix->d_fz_len);
	}
	if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream_fz) != hipSuccess) {
		bk_aux_free(ix);
		set_error("k_bk_aux failed");
		return -1;
	}
	ix->n_fz = n_c;
	return 0;
}

/* ---- fuzzy ----------------------------------------------------------- */

/*
 * Match-first search of all tokens at once (tokens of <= 64 bytes only), in two halves: mf_launch
 * queues the upload, the kernels and the copy back on stream_fz and returns (0 / -1); mf_finish waits
 * for them: 0 = term_ids filled, 1 = a queue overflowed (the caller takes the level-by-level
 * search), -1 = error.  Between the two the pass owns the fuzzy workspaces (fz, fz_pin).
 */
static int
mf_launch(nxsgpu_index_t *ix, int slot, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tok)
{
	nxsgpu_index::fz_slot_t &sl = ix->fzs[slot];
	const uint32_t n_c = ix->n_fz;
	const uint32_t blen = tok_off[n_tok] - tok_off[0];
	/* FZ_NQ sub-queues of qcap survivors each */
	/* (what a sub-queue can receive at most: its workgroups x 256 nodes x the
	 * tokens of a grid.y slice -- a small tree fills few sub-queues) */
	const uint32_t gy = std::max<uint32_t>(1, std::min<uint32_t>(8, n_tok / 128));
	const uint64_t q_most = (uint64_t)gy * (((n_c + 255) / 256 + FZ_NQ - 1) / FZ_NQ) * 256 * ((n_tok + gy - 1) / gy);
	const uint64_t qcap = std::min<uint64_t>(0xffffffffu, std::max<uint64_t>((n_tok + FZ_NQ - 1) / FZ_NQ + 1,
	    std::min<uint64_t>(ix->cfg.fuzzy_cand / FZ_NQ, q_most)));
	const uint64_t ccap = qcap * FZ_NQ;
	const uint64_t mcap = std::max<uint64_t>(1024, ccap / 4);
	const size_t need = 16384 + FZ_NQ * FZ_CSTRIDE * 4 + (ccap + mcap) * sizeof(fz_item_t) + (size_t)n_tok * (256 * 8 + 8 + 4 + 4 + 4) + 64 + blen + 16 +
	    ((size_t)n_tok + 1) * 4 + (NXS_MYERS_MAXPAT + 4) * 4 + 16 * 256 + 256;
	/* ONE upload from pinned memory -- token offsets, rank of every token in the length-sorted order, first
	 * rank of every length, then the tokens' bytes -- and ONE copy back (term ids, counters, evaluation counts):
	 * a copy to or from pageable memory is staged by the runtime and costs the host 20-40 us apiece, and the
	 * caller (plan_batch) sits waiting for this pass */
	const size_t up_words = (size_t)n_tok + 1 + n_tok + NXS_MYERS_MAXPAT + 2;
	const size_t up_bytes = (up_words * 4 + 15) & ~(size_t)15;
	const size_t dn_bytes = ((size_t)n_tok * 4 + 15 & ~(size_t)15) + 16 + 16;
	const size_t qcnt_bytes = (size_t)FZ_NQ * FZ_CSTRIDE * 4;	/* (copied back with the rest when profiling) */
	const size_t pin_need = up_bytes + blen + 16 + dn_bytes + qcnt_bytes + 64;
	if (sl.pin_len < pin_need) {
		if (sl.pin) {
			(void)hipHostFree(sl.pin);
			sl.pin = NULL;
			sl.pin_len = 0;
		}
		if (hipHostMalloc((void **)&sl.pin, pin_need + pin_need / 2, hipHostMallocDefault) != hipSuccess) {
			set_error("hipHostMalloc(%zu) for the fuzzy staging failed", pin_need);
			return -1;
		}
		sl.pin_len = pin_need + pin_need / 2;
	}
	uint32_t *const up = (uint32_t *)sl.pin;
	uint8_t *const h_dn = sl.pin + up_bytes + ((blen + 16 + 15) & ~(size_t)15);
	uint32_t *roff = up, *rank = roff + n_tok + 1, *len_off = rank + n_tok;

	if (sl.ws_len < need) {
		if (sl.ws) {
			(void)hipFree(sl.ws);
			sl.ws = NULL;
			sl.ws_len = 0;
		}
		if (hipMalloc(&sl.ws, need) != hipSuccess) {
			set_error("hipMalloc(%zu) for the fuzzy workspace failed", need);
			return -1;
		}
		sl.ws_len = need;
	}
	uint8_t *p = (uint8_t *)sl.ws;
	fz_item_t *d_cand = carve<fz_item_t>(p, ccap);
	fz_item_t *d_match = carve<fz_item_t>(p, mcap);
	/* (what comes back, in one piece: term ids | counters | evaluation counts; the sub-queue counters behind
	 * them are zeroed with the same memset) */
	uint8_t *d_dn = carve<uint8_t>(p, dn_bytes + FZ_NQ * FZ_CSTRIDE * 4);
	uint32_t *d_tids = (uint32_t *)d_dn;
	uint32_t *d_cnt = (uint32_t *)(d_dn + (((size_t)n_tok * 4 + 15) & ~(size_t)15));	/* -, matches, overflow, (seed's count) */
	unsigned long long *d_evals = (unsigned long long *)(d_cnt + 4);	/* distance evaluations, pairs compared */
	uint32_t *d_qcnt = (uint32_t *)(d_evals + 2);		/* survivors per sub-queue */
	uint64_t *d_peq = carve<uint64_t>(p, (size_t)n_tok * 256);
	uint2 *d_tokf = carve<uint2>(p, (size_t)n_tok + 4);
	uint32_t *d_best = carve<uint32_t>(p, n_tok);
	/* (what goes up, in one piece: the offset / rank / length words, then the bytes) */
	uint8_t *d_upb = carve<uint8_t>(p, up_bytes + blen + 16);
	uint32_t *d_up = (uint32_t *)d_upb;
	uint8_t *d_bytes = d_upb + up_bytes;
	uint32_t *d_off = d_up, *d_rank = d_up + n_tok + 1, *d_len_off = d_rank + n_tok;
	hipStream_t st = ix->stream_fz;
	fz_args_t fa;

#ifdef NXS_DBG_FZT
	static double acc[8]; static int ncall;
	auto nowd = []() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; };
	double tt = nowd();
#define FZT(i) do { double n_ = nowd(); acc[i] += n_ - tt; tt = n_; } while (0)
#else
#define FZT(i) do { } while (0)
#endif
	for (uint32_t i = 0; i <= n_tok; i++) {
		roff[i] = tok_off[i] - tok_off[0];
	}
	for (uint32_t l = 0; l <= NXS_MYERS_MAXPAT + 1; l++) {
		len_off[l] = 0;
	}
	for (uint32_t i = 0; i < n_tok; i++) {
		len_off[roff[i + 1] - roff[i] + 1]++;		/* (every token is <= 64 bytes here) */
	}
	for (uint32_t l = 0; l <= NXS_MYERS_MAXPAT; l++) {
		len_off[l + 1] += len_off[l];
	}
	{
		uint32_t next[NXS_MYERS_MAXPAT + 2];
		memcpy(next, len_off, sizeof(next));
		for (uint32_t i = 0; i < n_tok; i++) {
			rank[i] = next[roff[i + 1] - roff[i]]++;
		}
	}
	memcpy(sl.pin + up_bytes, tok_bytes + tok_off[0], blen);
	FZT(0);
	if (hipMemcpyAsync(d_upb, sl.pin, up_bytes + blen, hipMemcpyHostToDevice, st) != hipSuccess) {
		set_error("fuzzy upload failed");
		return -1;
	}
	FZT(1);
	if (hipMemsetAsync(d_cnt, 0, 16 + 16 + FZ_NQ * FZ_CSTRIDE * 4, st) != hipSuccess ||
	    hipMemsetAsync(d_tokf + n_tok, 0xff, 4 * sizeof(uint2), st) != hipSuccess) {
		set_error("fuzzy upload failed");
		return -1;
	}
	FZT(2);
	if (ix->profiling) (void)hipEventRecord(sl.ev[0], st);
	hipLaunchKernelGGL(k_bk_peq, dim3(n_tok), dim3(256), 0, st, d_bytes, d_off, n_tok, d_peq, d_tokf, d_rank);
	hipLaunchKernelGGL(k_bk_seed, dim3((n_tok + 255) / 256), dim3(256), 0, st, d_cand, d_cnt + 3, n_tok, d_best,
	    (unsigned long long *)NULL);
	if (n_c) {
		hipLaunchKernelGGL(k_fz_filter, dim3((n_c + 255) / 256, gy), dim3(256), 0, st,
		    ix->d_fz_sig, ix->d_fz_node, ix->d_fz_len, n_c, d_tokf, d_len_off, d_cand, d_qcnt,
		    (uint32_t)qcap, d_cnt + 2);
	}
	if (ix->profiling) (void)hipEventRecord(sl.ev[2], st);
	memset(&fa, 0, sizeof(fa));
	fa.bk = ix->d_bk;
	fa.bk_bytes = ix->d_bk_bytes;
	fa.tok_bytes = d_bytes;
	fa.tok_off = d_off;
	fa.peq = d_peq;
	fa.cap = (uint32_t)std::min<uint64_t>(ccap, 0xffffffffu);
	fa.best = d_best;
	fa.overflow = d_cnt + 2;
	fa.prune = 1;
	fa.evals = ix->profiling ? d_evals : NULL;
	hipLaunchKernelGGL(k_fz_dist, dim3(8, FZ_NQ), dim3(1024), 0, st, fa, d_cand, d_qcnt, (uint32_t)qcap, d_match, d_cnt + 1,
	    (uint32_t)std::min<uint64_t>(mcap, 0xffffffffu));
	if (ix->profiling) (void)hipEventRecord(sl.ev[3], st);
	hipLaunchKernelGGL(k_fz_chain, dim3(1024), dim3(256), 0, st, fa, ix->d_bk_parent, ix->d_bk_slot, d_match, d_cnt + 1,
	    (uint32_t)std::min<uint64_t>(mcap, 0xffffffffu));
	hipLaunchKernelGGL(k_bk_finish, dim3((n_tok + 255) / 256), dim3(256), 0, st, ix->d_bk, d_best, n_tok, d_tids);
	if (ix->profiling) (void)hipEventRecord(sl.ev[1], st);
	if (hipGetLastError() != hipSuccess) {
		set_error("fuzzy kernel launch failed");
		return -1;
	}
	FZT(3);
#ifdef NXS_DBG_FZT
	if (++ncall % 200 == 0) fprintf(stderr, "fzt host %.1f up %.1f memset %.1f kernels %.1f us (prof %d)\n", 1e6*acc[0]/ncall, 1e6*acc[1]/ncall, 1e6*acc[2]/ncall, 1e6*acc[3]/ncall, (int)ix->profiling);
#endif
	/* (one copy into PINNED memory: a copy to pageable memory makes the call wait for the stream) */
	if (hipMemcpyAsync(h_dn, d_dn, dn_bytes + (ix->profiling ? qcnt_bytes : 0), hipMemcpyDeviceToHost, st) != hipSuccess) {
		set_error("fuzzy pass failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	/* (the pass's own end: another pass may be queued behind it on the stream before this one is waited for) */
	if (hipEventRecord(sl.ev_done, st) != hipSuccess) {
		set_error("fuzzy pass failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	return 0;
}

static int
mf_finish(nxsgpu_index_t *ix, int slot, uint32_t n_tok, uint32_t *term_ids)
{
	nxsgpu_index::fz_slot_t &sl = ix->fzs[slot];
	/* (the staging layout of mf_launch) */
	const uint32_t n_c = ix->n_fz;
	const size_t up_words = (size_t)n_tok + 1 + n_tok + NXS_MYERS_MAXPAT + 2;
	const size_t up_bytes = (up_words * 4 + 15) & ~(size_t)15;
	const uint32_t *const len_off = (const uint32_t *)sl.pin + n_tok + 1 + n_tok;
	const uint32_t blen = ((const uint32_t *)sl.pin)[n_tok];
	const uint8_t *const h_dn = sl.pin + up_bytes + ((blen + 16 + 15) & ~(size_t)15);
	const size_t dn_bytes = ((size_t)n_tok * 4 + 15 & ~(size_t)15) + 16 + 16;
	const uint32_t *const h_qcnt = (const uint32_t *)(h_dn + dn_bytes);	/* (valid when profiling) */

	if (hipEventSynchronize(sl.ev_done) != hipSuccess) {
		set_error("fuzzy pass failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	const uint32_t *const h_cnt = (const uint32_t *)(h_dn + (((size_t)n_tok * 4 + 15) & ~(size_t)15));
	const unsigned long long *const h_evals = (const unsigned long long *)(h_cnt + 4);
	memcpy(term_ids, h_dn, (size_t)n_tok * 4);
	if (ix->profiling) {
		float ms = 0;
		(void)hipEventElapsedTime(&ms, sl.ev[0], sl.ev[1]);
		ix->prof.fuzzy_ms += ms;
		(void)hipEventElapsedTime(&ms, sl.ev[0], sl.ev[2]);
		ix->prof.fuzzy_filter_ms += ms;
		(void)hipEventElapsedTime(&ms, sl.ev[2], sl.ev[3]);
		ix->prof.fuzzy_dist_ms += ms;
		(void)hipEventElapsedTime(&ms, sl.ev[3], sl.ev[1]);
		ix->prof.fuzzy_chain_ms += ms;
	}
	if (h_cnt[2]) {
		return 1;
	}
	if (ix->profiling) {
		/* distance evaluations; "pairs" = what the queues carried; levels: pairs
		 * screened, survivors, matches */
		uint64_t surv = 0;
		for (uint32_t q = 0; q < FZ_NQ; q++) {
			surv += h_qcnt[q * FZ_CSTRIDE];
		}
		ix->prof.fuzzy_visits += h_evals[0];
		/* the (token, term) pairs k_fz_filter compared: per workgroup of 256 candidates
		 * (sorted by length) the tokens of compatible length -- the kernel's own bounds */
		if (ix->fz_len_start.size() == FZ_MAXLEN + 2) {
			uint64_t checked = 0;
			uint32_t l_lo = 0, l_hi = 0;
			for (uint32_t first = 0; first < n_c; first += 256) {
				const uint32_t last = std::min(first + 255, n_c - 1);
				while (ix->fz_len_start[l_lo + 1] <= first) l_lo++;
				l_hi = std::max(l_hi, l_lo);
				while (ix->fz_len_start[l_hi + 1] <= last) l_hi++;
				const uint32_t ta = len_off[l_lo > 2 ? l_lo - 2 : 0];
				const uint32_t tb = len_off[std::min<uint32_t>(l_hi + 2, NXS_MYERS_MAXPAT) + 1];
				checked += (uint64_t)(last - first + 1) * (tb > ta ? tb - ta : 0);
			}
			ix->prof.fuzzy_checked += checked;
		}
		ix->prof.fuzzy_pairs += surv + h_cnt[1];
		ix->prof.fuzzy_level[0] += (uint64_t)n_tok * n_c;
		ix->prof.fuzzy_level[1] += surv;
		ix->prof.fuzzy_level[2] += h_cnt[1];
	}
	return 0;
}

/* can the batch take the match-first pass as ONE launch sequence (the usual case: no visit counts wanted,
 * every token fits the bit-vector distance)? */
static bool
mf_whole_batch(const nxsgpu_index_t *ix, const uint32_t *tok_off, uint32_t n_tok)
{
	if (ix->cfg.fuzzy_bfs || ix->cfg.fuzzy_noprune || !ix->d_bk_parent || !ix->n_bk || !n_tok) {
		return false;
	}
	for (uint32_t i = 0; i < n_tok; i++) {
		if (tok_off[i + 1] - tok_off[i] > NXS_MYERS_MAXPAT) {
			return false;
		}
	}
	return true;
}

static int fuzzy_search(nxsgpu_index_t *, const uint8_t *, const uint32_t *, uint32_t, uint32_t *, uint64_t *, bool);

static int
mf_free_slot(const nxsgpu_index_t *ix)
{
	for (int i = 0; i < NXSGPU_FZ_SLOTS; i++) {
		if (!ix->fzs[i].state) {
			return i;
		}
	}
	return -1;
}

extern "C" int
nxsgpu_fuzzy(nxsgpu_index_t *ix, const uint8_t *tok_bytes, const uint32_t *tok_off,
    uint32_t n_tok, uint32_t *term_ids, uint64_t *visited)
{
	for (int i = 0; i < NXSGPU_FZ_SLOTS; i++) {
		if (ix->fzs[i].state) {
			set_error("a fuzzy pass is in flight (nxsgpu_fuzzy_begin without _end)");
			return -1;
		}
	}
	return fuzzy_search(ix, tok_bytes, tok_off, n_tok, term_ids, visited, false);
}

/*
 * The same search in two calls: _begin queues the match-first pass of the whole batch on the fuzzy stream
 * and returns a slot (>= 0; -1: error, -2: both slots are taken); _end (slot, same tokens) waits for it
 * and delivers the term ids -- or runs the level-by-level search when a queue of the pass overflowed, and
 * the whole search when the batch did not qualify for a single pass.  NXSGPU_FZ_SLOTS passes can be in
 * flight, each with workspaces of its own; they run in the order they were begun and are to be ended in
 * that order.  nxsgpu_fuzzy() refuses to run meanwhile.
 */
extern "C" int
nxsgpu_fuzzy_begin(nxsgpu_index_t *ix, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tok)
{
	const int slot = mf_free_slot(ix);

	if (slot < 0) {
		set_error("%d fuzzy passes are in flight already", NXSGPU_FZ_SLOTS);
		return -2;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	ix->fzs[slot].n = n_tok;
	if (!mf_whole_batch(ix, tok_off, n_tok)) {
		ix->fzs[slot].state = 2;
		return slot;
	}
	if (mf_launch(ix, slot, tok_bytes, tok_off, n_tok) != 0) {
		(void)hipStreamSynchronize(ix->stream_fz);
		return -1;
	}
	ix->fzs[slot].state = 1;
	return slot;
}

extern "C" int
nxsgpu_fuzzy_end(nxsgpu_index_t *ix, int slot, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tok,
    uint32_t *term_ids)
{
	if (slot < 0 || slot >= NXSGPU_FZ_SLOTS || !ix->fzs[slot].state || n_tok != ix->fzs[slot].n) {
		set_error("nxsgpu_fuzzy_end without a matching _begin");
		return -1;
	}
	const int mode = ix->fzs[slot].state;
	if (hipSetDevice(ix->device) != hipSuccess) {
		ix->fzs[slot].state = 0;
		set_error("hipSetDevice failed");
		return -1;
	}
	if (mode == 1) {
		const int r = mf_finish(ix, slot, n_tok, term_ids);
		ix->fzs[slot].state = 0;
		if (r <= 0) {
			return r;
		}
		return fuzzy_search(ix, tok_bytes, tok_off, n_tok, term_ids, NULL, true);
	}
	ix->fzs[slot].state = 0;
	return fuzzy_search(ix, tok_bytes, tok_off, n_tok, term_ids, NULL, false);
}

/* (no_mf: the match-first pass of these tokens has been tried and overflowed) */
static int
fuzzy_search(nxsgpu_index_t *ix, const uint8_t *tok_bytes, const uint32_t *tok_off,
    uint32_t n_tok, uint32_t *term_ids, uint64_t *visited, bool no_mf)
{
	const uint64_t budget = ix->cfg.fuzzy_items;
	const uint32_t n_bk = ix->n_bk;
	uint32_t chunk, max_len = 0;
	bool any_long = false;

	if (n_tok == 0) {
		return 0;
	}
	if (n_bk == 0) {
		memset(term_ids, 0, n_tok * sizeof(uint32_t));
		if (visited) memset(visited, 0, n_tok * sizeof(uint64_t));
		return 0;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	for (uint32_t i = 0; i < n_tok; i++) {
		const uint32_t m = tok_off[i + 1] - tok_off[i];
		max_len = std::max(max_len, m);
		if (m > NXS_MYERS_MAXPAT) {
			any_long = true;
		}
	}
	/*
	 * Worst case one token visits every node: with `safe_chunk` tokens per pass
	 * the frontier queues can never overflow.  A d <= 2 search visits ~10 % of a
	 * large tree, though, so the whole batch is tried in ONE pass first (29
	 * level launches instead of 29 per chunk, and fuller levels); a pass that
	 * does overflow the queues is repeated with a quarter of the tokens, down to
	 * the safe size.
	 */
	/* the usual case: no visit counts wanted, every token fits the bit-vector
	 * distance -- match first, then reachability; the frontier search below is
	 * what the reference does, step for step, and the fallback */
	if (!visited && !no_mf && !ix->cfg.fuzzy_bfs && !ix->cfg.fuzzy_noprune && ix->d_bk_parent) {
		if (!any_long) {
			/* (a free slot: nxsgpu_fuzzy() runs with none taken, nxsgpu_fuzzy_end() has given its own back) */
			const int slot = mf_free_slot(ix);
			int r = slot < 0 ? 1 : mf_launch(ix, slot, tok_bytes, tok_off, n_tok);
			if (slot >= 0 && r == 0) {
				r = mf_finish(ix, slot, n_tok, term_ids);
			} else if (slot >= 0) {
				(void)hipStreamSynchronize(ix->stream_fz);
			}
			if (r <= 0) {
				return r;
			}
		} else if (!ix->fz_split) {
			/* tokens beyond the bit-vector distance (> 64 bytes) take the frontier
			 * search with its row DP, the others the match-first search */
			std::vector<uint32_t> sel[2], off[2], ids[2];
			std::vector<uint8_t> bytes[2];
			int rc = 0;
			for (uint32_t i = 0; i < n_tok; i++) {
				const uint32_t m = tok_off[i + 1] - tok_off[i];
				const int w = m > NXS_MYERS_MAXPAT;
				if (sel[w].empty()) {
					off[w].push_back(0);
				}
				sel[w].push_back(i);
				bytes[w].insert(bytes[w].end(), tok_bytes + tok_off[i], tok_bytes + tok_off[i + 1]);
				off[w].push_back((uint32_t)bytes[w].size());
			}
			ix->fz_split = true;
			for (int w = 0; w < 2 && rc == 0; w++) {
				if (!sel[w].empty()) {
					ids[w].resize(sel[w].size());
					bytes[w].resize(bytes[w].size() + 16);
					rc = fuzzy_search(ix, bytes[w].data(), off[w].data(), (uint32_t)sel[w].size(), ids[w].data(), NULL, false);
					for (size_t j = 0; j < sel[w].size(); j++) {
						term_ids[sel[w][j]] = ids[w][j];
					}
				}
			}
			ix->fz_split = false;
			return rc;
		}
	}
	const uint32_t safe_chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_tok, budget / n_bk));
	chunk = ix->cfg.fuzzy_safe ? safe_chunk : n_tok;

	const uint32_t LONG_THREADS = 64 * 64;
	const uint64_t cap = std::max<uint64_t>((uint64_t)safe_chunk * n_bk, std::min<uint64_t>(budget, (uint64_t)chunk * n_bk));
	const size_t levels = (size_t)ix->bk_depth + 2;
	size_t need = 4096 + cap * sizeof(fz_item_t) * 2 + levels * 4 + 256
	    + (size_t)chunk * (256 * 8 + 4 + 8 + 4) + tok_off[n_tok] + 16 + ((size_t)chunk + 1) * 4 + 512
	    + (any_long ? (size_t)LONG_THREADS * ((size_t)max_len + 2) * 2 : 0) + 16 * 256;
	if (ix->fz_len < need) {
		if (ix->fz) {
			(void)hipFree(ix->fz);
			ix->fz = NULL;
			ix->fz_len = 0;
		}
		if (hipMalloc(&ix->fz, need) != hipSuccess) {
			set_error("hipMalloc(%zu) for the fuzzy workspace failed", need);
			return -1;
		}
		ix->fz_len = need;
	}

	for (uint32_t c0 = 0; c0 < n_tok; ) {
		const uint32_t nc = std::min(chunk, n_tok - c0);
		const uint32_t boff = tok_off[c0], blen = tok_off[c0 + nc] - boff;
		std::vector<uint32_t> roff(nc + 1);
		uint8_t *p = (uint8_t *)ix->fz;
		fz_item_t *qa = carve<fz_item_t>(p, cap);
		fz_item_t *qb = carve<fz_item_t>(p, cap);
		uint32_t *counts = carve<uint32_t>(p, levels);
		uint32_t *d_ovf = carve<uint32_t>(p, 1);
		uint64_t *d_peq = carve<uint64_t>(p, (size_t)nc * 256);
		uint32_t *d_best = carve<uint32_t>(p, nc);
		unsigned long long *d_vis = carve<unsigned long long>(p, nc);
		unsigned long long *d_evals = carve<unsigned long long>(p, 1);
		uint32_t *d_tids = carve<uint32_t>(p, nc);
		uint8_t *d_bytes = carve<uint8_t>(p, blen + 16);
		uint32_t *d_off = carve<uint32_t>(p, nc + 1);
		uint16_t *d_rows = any_long ? carve<uint16_t>(p, (size_t)LONG_THREADS * (max_len + 2)) : NULL;
		fz_args_t fa;
		uint32_t h_ovf = 0;

		for (uint32_t i = 0; i <= nc; i++) {
			roff[i] = tok_off[c0 + i] - boff;
		}
		if (hipMemcpyAsync(d_bytes, tok_bytes + boff, blen, hipMemcpyHostToDevice, ix->stream_fz) != hipSuccess ||
		    hipMemcpyAsync(d_off, roff.data(), (nc + 1) * 4, hipMemcpyHostToDevice, ix->stream_fz) != hipSuccess ||
		    hipMemsetAsync(counts, 0, levels * 4, ix->stream_fz) != hipSuccess ||
		    hipMemsetAsync(d_ovf, 0, 4, ix->stream_fz) != hipSuccess ||
		    hipMemsetAsync(d_evals, 0, 8, ix->stream_fz) != hipSuccess) {
			set_error("fuzzy upload failed");
			return -1;
		}
		if (ix->profiling) (void)hipEventRecord(ix->ev[0], ix->stream_fz);
		hipLaunchKernelGGL(k_bk_peq, dim3(nc), dim3(256), 0, ix->stream_fz, d_bytes, d_off, nc, d_peq, (uint2 *)NULL, (const uint32_t *)NULL);
		hipLaunchKernelGGL(k_bk_seed, dim3((nc + 255) / 256), dim3(256), 0, ix->stream_fz,
		    qa, counts, nc, d_best, visited ? d_vis : (unsigned long long *)NULL);

		memset(&fa, 0, sizeof(fa));
		fa.bk = ix->d_bk;
		fa.bk_bytes = ix->d_bk_bytes;
		fa.tok_bytes = d_bytes;
		fa.tok_off = d_off;
		fa.peq = d_peq;
		fa.cap = (uint32_t)std::min<uint64_t>(cap, 0xffffffffu);
		fa.best = d_best;
		fa.visited = visited ? d_vis : NULL;
		fa.dp_rows = d_rows;
		fa.dp_stride = max_len + 2;
		fa.overflow = d_ovf;
		fa.prune = (!visited && !ix->cfg.fuzzy_noprune) ? 1u : 0u;
		fa.evals = ix->profiling ? d_evals : NULL;
		for (uint32_t lvl = 0; lvl < ix->bk_depth; lvl++) {
			fa.cur = (lvl & 1) ? qb : qa;
			fa.next = (lvl & 1) ? qa : qb;
			fa.cur_count = counts + lvl;
			fa.next_count = counts + lvl + 1;
			hipLaunchKernelGGL(k_bk_level<false>, dim3(512), dim3(1024), 0, ix->stream_fz, fa);
			if (any_long) {
				/* tokens longer than 64 bytes: row DP, bounded scratch */
				hipLaunchKernelGGL(k_bk_level<true>, dim3(LONG_THREADS / 64), dim3(64), 0, ix->stream_fz, fa);
			}
		}
		hipLaunchKernelGGL(k_bk_finish, dim3((nc + 255) / 256), dim3(256), 0, ix->stream_fz,
		    ix->d_bk, d_best, nc, d_tids);
		if (ix->profiling) (void)hipEventRecord(ix->ev[1], ix->stream_fz);
		if (hipGetLastError() != hipSuccess) {
			set_error("fuzzy kernel launch failed");
			return -1;
		}
		std::vector<uint32_t> h_counts(levels);
		unsigned long long h_evals = 0;
		if (hipMemcpyAsync(term_ids + c0, d_tids, nc * 4, hipMemcpyDeviceToHost, ix->stream_fz) != hipSuccess ||
		    hipMemcpyAsync(&h_evals, d_evals, 8, hipMemcpyDeviceToHost, ix->stream_fz) != hipSuccess ||
		    (visited && hipMemcpyAsync(visited + c0, d_vis, nc * 8, hipMemcpyDeviceToHost, ix->stream_fz) != hipSuccess) ||
		    hipMemcpyAsync(&h_ovf, d_ovf, 4, hipMemcpyDeviceToHost, ix->stream_fz) != hipSuccess ||
		    hipMemcpyAsync(h_counts.data(), counts, levels * 4, hipMemcpyDeviceToHost, ix->stream_fz) != hipSuccess ||
		    hipStreamSynchronize(ix->stream_fz) != hipSuccess) {
			set_error("fuzzy pass failed: %s", hipGetErrorString(hipGetLastError()));
			return -1;
		}
		if (ix->profiling) {
			float ms = 0;
			(void)hipEventElapsedTime(&ms, ix->ev[0], ix->ev[1]);
			ix->prof.fuzzy_ms += ms;		/* a repeated pass is time spent too */
		}
		if (h_ovf) {
			if (chunk <= safe_chunk) {
				set_error("fuzzy frontier overflow (internal error)");
				return -1;
			}
			chunk = std::max(safe_chunk, chunk / 4);
			continue;		/* same tokens again, fewer at a time */
		}
		if (ix->profiling) {
			/* distance evaluations; (token, node) pairs dequeued, pruned ones
			 * included, are the level counts */
			ix->prof.fuzzy_visits += h_evals;
			for (size_t l = 0; l < levels; l++) {
				ix->prof.fuzzy_pairs += h_counts[l];
				if (l < 40) {
					ix->prof.fuzzy_level[l] += h_counts[l];
				}
			}
		}
		c0 += nc;
	}
	return 0;
}

/* ---- spelling suggestions -------------------------------------------- */
/*
 * nxsgpu_suggest: for every token the dictionary terms within maxdist (1 or 2) that have a posting in a
 * live doc, best k by (distance ascending, df descending, term id ascending), and how many there are.
 *
 * The match-first search above already screens every (token, term) pair and takes the exact distance of
 * every survivor; it keeps the one term bktree_search would pick.  This pass keeps them all:
 *
 *   candidates   a permutation of its own beside d_fz_node: every node whose term has df > 0 (the CSR's
 *                live posting count) and at most FZ_MAXLEN bytes -- whether or not the BK walk reaches it
 *                (slot-63 subtrees) and whatever the on-disk total says -- sorted by length; built on the
 *                first call and again when nxsgpu_index::sg_gen has moved
 *   k_fz_filter  unchanged, on those arrays: survivors into the FZ_NQ sub-queues
 *   k_sg_dist    exact distance; d <= maxdist bumps the token's counter and appends (token, d, node) to
 *                the match queue (one returning atomic per workgroup and round)
 *   k_sg_scan    exclusive scan of the counters: a segment per token
 *   k_sg_scatter the queue into the segments, as sort keys: d << 32 | ~df, term id
 *   k_sg_select  one wavefront per token, k rounds of a wave-wide minimum over the segment (the keys are
 *                distinct: a total order, so the result does not depend on queue order)
 *
 * A queue that overflows is never a wrong answer: the pass is repeated with a quarter of the tokens, and
 * a single token that still overflows gets queues sized to what the screen can emit at most (8 bytes x
 * candidates).  Tokens beyond the bit-vector distance and everything under NXS_GPU_SUGGEST=host take the
 * host ranker (nxs_suggest.h) over a host copy of the BK image.
 */
#include "nxs_suggest.h"

struct sg_key_t { uint64_t hi, lo; };		/* d << 32 | ~df, term id */

struct sg_state_t {
	side_t		side;
	bool		built;
	uint64_t	built_gen;
	uint32_t *	d_node;		/* [n_c] candidates, sorted by term length */
	uint32_t *	d_sig;
	uint8_t *	d_len;
	uint32_t	n_c;
	dict_host_t	dict;		/* the host ranker's dictionary: every node with df > 0, any length */
	double		prof[NXSGPU_SUGGEST_PROF];
};

#define	SG_TOK_BITS	30
#define	SG_TOK_MASK	((1u << SG_TOK_BITS) - 1)

__global__ void __launch_bounds__(1024)
k_sg_dist(const fz_args_t A, const fz_item_t *cand, const uint32_t *cand_count, uint32_t qcap, uint32_t maxdist,
    uint32_t *tok_matches, uint2 *match, uint32_t *match_count, uint32_t mcap)
{
	__shared__ uint32_t s_wtot[16], s_base;
	const unsigned wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
	const uint32_t count = min(cand_count[blockIdx.y * FZ_CSTRIDE], qcap);
	const uint32_t nthreads = gridDim.x * blockDim.x;
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t rounds = (count + nthreads - 1) / nthreads;

	cand += (uint64_t)blockIdx.y * qcap;
	for (uint32_t r = 0; r < rounds; r++) {
		const uint32_t i = r * nthreads + tid;
		uint2 mi = make_uint2(0, 0);
		bool hit = false;

		if (i < count) {
			const fz_item_t it = cand[i];
			const nxsgpu_bknode_t nd = A.bk[it.node];
			const int d = fz_distance(A, it.tok, nd, 0);
			if ((uint32_t)d <= maxdist) {
				hit = true;
				mi = make_uint2(it.tok | ((uint32_t)d << SG_TOK_BITS), it.node);
				atomicAdd(&tok_matches[it.tok], 1u);
			}
		}
		const uint64_t m = ballot64(hit);
		s_wtot[wid] = __popcll(m);
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t sum = 0;
			for (unsigned w = 0; w < nw; w++) {
				const uint32_t tw = s_wtot[w];
				s_wtot[w] = sum;
				sum += tw;
			}
			s_base = sum ? atomicAdd(match_count, sum) : 0;
		}
		__syncthreads();
		const uint32_t o = s_base + s_wtot[wid] + lanes_below(m);
		__syncthreads();
		if (hit) {
			if (o < mcap) {
				match[o] = mi;
			} else {
				*A.overflow = 1;
			}
		}
	}
}

/* seg_off[i] = sum of cnt[0 .. i), seg_off[n] = the total; fill[] = 0 (one workgroup) */
__global__ void __launch_bounds__(1024)
k_sg_scan(const uint32_t *cnt, uint32_t n, uint32_t *seg_off, uint32_t *fill)
{
	__shared__ uint32_t s_w[16], s_carry;
	const unsigned lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

	if (threadIdx.x == 0) {
		s_carry = 0;
	}
	__syncthreads();
	for (uint32_t base = 0; base < n; base += 1024) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n ? cnt[i] : 0;
		uint32_t incl = v, woff = 0;
		for (int o = 1; o < WAVE; o <<= 1) {
			const uint32_t u = (uint32_t)__shfl_up((int)incl, o);
			if (lane >= (unsigned)o) incl += u;
		}
		if (lane == WAVE - 1) {
			s_w[wid] = incl;
		}
		__syncthreads();
		for (unsigned w = 0; w < wid; w++) {
			woff += s_w[w];
		}
		const uint32_t carry = s_carry;
		if (i < n) {
			seg_off[i] = carry + woff + incl - v;
			fill[i] = 0;
		}
		__syncthreads();
		if (threadIdx.x == 1023) {
			s_carry = carry + woff + incl;
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		seg_off[n] = s_carry;
	}
}

/* the match queue into the tokens' segments, as sort keys; df = the CSR's live posting count */
__global__ void __launch_bounds__(256)
k_sg_scatter(const nxsgpu_bknode_t *__restrict__ bk, const uint64_t *__restrict__ post_off, uint32_t n_terms,
    const uint2 *__restrict__ match, const uint32_t *__restrict__ match_count, uint32_t mcap,
    const uint32_t *__restrict__ seg_off, uint32_t *fill, sg_key_t *keys)
{
	const uint32_t count = min(*match_count, mcap);
	const uint32_t nthreads = gridDim.x * blockDim.x;

	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += nthreads) {
		const uint2 m = match[i];
		const uint32_t tok = m.x & SG_TOK_MASK, d = m.x >> SG_TOK_BITS;
		const uint32_t term = bk[m.y].term_id;
		const uint32_t df = (term >= 1 && term <= n_terms) ? (uint32_t)(post_off[term + 1] - post_off[term]) : 0;
		const uint32_t pos = seg_off[tok] + atomicAdd(&fill[tok], 1u);
		sg_key_t key;

		key.hi = ((uint64_t)d << 32) | (uint32_t)~df;
		key.lo = term;
		/* (inside the segment always; inside the array unless the match queue overflowed: that pass's
		 * counters say more than the queue holds, and its rows are discarded) */
		if (pos < seg_off[tok + 1] && pos < mcap) {
			keys[pos] = key;
		}
	}
}

static __device__ __forceinline__ bool
sg_less(const sg_key_t &a, const sg_key_t &b)
{
	return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo);
}

/*
 * One wavefront per token: round r delivers the r-th smallest key of the segment -- the smallest one
 * above the previous round's (the keys are distinct: a term appears once).  Every lane looks at its
 * stride of the segment (its first item stays in registers: segments of up to 64 matches, nearly all of
 * them, are read once), the 64 candidates meet in a butterfly.  Exact for segments of any length.
 */
__global__ void __launch_bounds__(64)
k_sg_select(const sg_key_t *__restrict__ keys, const uint32_t *__restrict__ seg_off, uint32_t mcap, uint32_t k,
    uint32_t *term_ids, uint8_t *dist, uint32_t *df, uint32_t *counts)
{
	const uint32_t tok = blockIdx.x;
	const unsigned lane = threadIdx.x;
	/* (a segment that ends beyond the array belongs to an overflowed pass: nothing to select) */
	const uint32_t s = seg_off[tok], e = seg_off[tok + 1], n = e <= mcap ? e - s : 0;
	const uint32_t nout = min(k, n);
	const sg_key_t none = { ~0ull, ~0ull };
	sg_key_t mine = none, prev = none;

	if (lane < n) {
		mine = keys[s + lane];
	}
	for (uint32_t r = 0; r < nout; r++) {
		sg_key_t best = none;

		if (lane < n && (r == 0 || sg_less(prev, mine))) {
			best = mine;
		}
		for (uint32_t i = lane + WAVE; i < n; i += WAVE) {
			const sg_key_t c = keys[s + i];
			if ((r == 0 || sg_less(prev, c)) && sg_less(c, best)) {
				best = c;
			}
		}
		for (int o = 32; o; o >>= 1) {
			sg_key_t c;
			c.hi = (uint64_t)__shfl_xor((long long)best.hi, o);
			c.lo = (uint64_t)__shfl_xor((long long)best.lo, o);
			if (sg_less(c, best)) {
				best = c;
			}
		}
		if (lane == 0) {
			const uint64_t at = (uint64_t)tok * k + r;
			term_ids[at] = (uint32_t)best.lo;
			dist[at] = (uint8_t)(best.hi >> 32);
			df[at] = ~(uint32_t)best.hi;
		}
		prev = best;
	}
	if (lane == 0) {
		counts[tok] = nout;
	}
}

void
sg_free(nxsgpu_index_t *ix)
{
	sg_state_t *sg = ix->sg;

	if (!sg) {
		return;
	}
	side_close(&sg->side, true);
	(void)hipFree(sg->d_node);
	(void)hipFree(sg->d_sig);
	(void)hipFree(sg->d_len);
	delete sg;
	ix->sg = NULL;
}

/* the state, and the candidates of the index's current generation */
static int
sg_prepare(nxsgpu_index_t *ix)
{
	if (!ix->sg) {
		ix->sg = new sg_state_t();
	}
	sg_state_t *sg = ix->sg;

	if (side_open(ix, &sg->side, "suggest", 5, true) != 0) {
		return -1;
	}
	if (sg->built && sg->built_gen == ix->sg_gen) {
		return 0;
	}
	sg->built = false;
	(void)hipFree(sg->d_node);
	(void)hipFree(sg->d_sig);
	(void)hipFree(sg->d_len);
	sg->d_node = sg->d_sig = NULL;
	sg->d_len = NULL;
	sg->n_c = 0;
	if (dict_host_build(ix, sg->side.st, &sg->dict, "suggest") != 0) {
		return -1;
	}
	/* the candidates: the dictionary's nodes (df > 0) of at most FZ_MAXLEN bytes, sorted by length */
	const std::vector<nxsgpu_bknode_t> &nodes = sg->dict.h_nodes;
	const uint32_t n = (uint32_t)nodes.size();
	auto cand = [&](uint32_t i) -> bool {
		return nodes[i].str_len <= FZ_MAXLEN && dict_df(ix->h_post_off.data(), ix->n_terms, nodes[i].term_id);
	};
	std::vector<uint32_t> start(FZ_MAXLEN + 2, 0), perm;
	uint32_t n_c = 0;
	for (uint32_t i = 0; i < n; i++) {
		if (cand(i)) {
			start[nodes[i].str_len + 1]++;
			n_c++;
		}
	}
	for (uint32_t l = 0; l <= FZ_MAXLEN; l++) {
		start[l + 1] += start[l];
	}
	perm.resize(std::max<uint32_t>(n_c, 1));
	for (uint32_t i = 0; i < n; i++) {
		if (cand(i)) {
			perm[start[nodes[i].str_len]++] = i;
		}
	}
	if (n_c) {
		if (hipMalloc(&sg->d_node, (size_t)n_c * 4) != hipSuccess ||
		    hipMalloc(&sg->d_sig, (size_t)n_c * 4) != hipSuccess ||
		    hipMalloc(&sg->d_len, (size_t)n_c + 16) != hipSuccess ||
		    hipMemcpyAsync(sg->d_node, perm.data(), (size_t)n_c * 4, hipMemcpyHostToDevice, sg->side.st) != hipSuccess) {
			set_error("suggest candidates: out of device memory");
			return -1;
		}
		hipLaunchKernelGGL(k_fz_sigs, dim3((n_c + 255) / 256), dim3(256), 0, sg->side.st,
		    ix->d_bk, ix->d_bk_bytes, sg->d_node, n_c, sg->d_sig, sg->d_len);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sg->side.st) != hipSuccess) {
			set_error("suggest candidates: k_fz_sigs failed");
			return -1;
		}
	}
	sg->n_c = n_c;
	sg->built = true;
	sg->built_gen = ix->sg_gen;
	return 0;
}

/*
 * One device pass over tokens [0, n_tok) (every one <= NXS_MYERS_MAXPAT bytes; tok_off[0] need not be 0):
 * one upload from pinned memory, the kernels, one copy back; blocking.  `full`: queues sized to what the
 * screen can emit at most.  0 = rows written, 1 = a queue overflowed (nothing written), -1 = error.
 */
static int
sg_pass(nxsgpu_index_t *ix, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tok, bool full,
    uint32_t maxdist, uint32_t k, const uint32_t *dest, uint32_t *o_ids, uint8_t *o_dist, uint32_t *o_df,
    uint32_t *o_counts, uint32_t *o_matches)
{
	sg_state_t *sg = ix->sg;
	const uint32_t n_c = sg->n_c;
	const uint32_t blen = tok_off[n_tok] - tok_off[0];
	const uint32_t gy = std::max<uint32_t>(1, std::min<uint32_t>(8, n_tok / 128));
	/* (what a sub-queue can receive at most: mf_launch) */
	const uint64_t q_most = (uint64_t)gy * (((n_c + 255) / 256 + FZ_NQ - 1) / FZ_NQ) * 256 * ((n_tok + gy - 1) / gy);
	const uint64_t qcap = std::min<uint64_t>(0xffffffffu / FZ_NQ, std::max<uint64_t>(16,
	    full ? q_most : std::min<uint64_t>(ix->cfg.fuzzy_cand / FZ_NQ, q_most)));
	const uint64_t ccap = qcap * FZ_NQ;
	/* (matches are survivors: a single token's match queue cannot overflow before its survivor queues do) */
	const uint64_t mcap = n_tok == 1 ? ccap : std::max<uint64_t>(1024, ccap / 4);
	const size_t rows = (size_t)n_tok * k;
	/* up: offsets | rank in the length-sorted order | first rank of every length | bytes (mf_launch) */
	const size_t up_words = (size_t)n_tok + 1 + n_tok + NXS_MYERS_MAXPAT + 2;
	const size_t up_bytes = (up_words * 4 + 15) & ~(size_t)15;
	/* down: term ids | df | counts | matches | counters (-, matches queued, overflow, -) | survivors per
	 * sub-queue | distances */
	const size_t dn_words = rows * 2 + (size_t)n_tok * 2 + 4 + FZ_NQ * FZ_CSTRIDE;
	const size_t dn_bytes = (dn_words * 4 + rows + 15) & ~(size_t)15;
	const size_t pin_need = up_bytes + ((blen + 16 + 15) & ~(size_t)15) + dn_bytes + 64;
	const size_t need = ccap * sizeof(fz_item_t) + mcap * (sizeof(uint2) + sizeof(sg_key_t)) + dn_bytes +
	    (size_t)n_tok * (256 * 8 + 8 + 4 + 4) + 64 + up_bytes + blen + 16 + 16 * 256;
	side_t *sd = &sg->side;
	hipStream_t st = sd->st;
	const bool prof = ix->profiling && sd->ev_ok;

	if (side_room(sd, "suggest", pin_need, need) != 0) {
		return -1;
	}
	uint32_t *const up = (uint32_t *)sd->pin;
	uint8_t *const h_dn = sd->pin + up_bytes + ((blen + 16 + 15) & ~(size_t)15);
	uint32_t *roff = up, *rank = roff + n_tok + 1, *len_off = rank + n_tok;

	uint8_t *p = (uint8_t *)sd->ws;
	fz_item_t *d_cand = carve<fz_item_t>(p, ccap);
	uint2 *d_match = carve<uint2>(p, mcap);
	sg_key_t *d_keys = carve<sg_key_t>(p, mcap);
	uint8_t *d_dn = carve<uint8_t>(p, dn_bytes);
	uint32_t *d_ids = (uint32_t *)d_dn, *d_df = d_ids + rows, *d_counts = d_df + rows, *d_matches = d_counts + n_tok;
	uint32_t *d_cnt = d_matches + n_tok, *d_qcnt = d_cnt + 4;
	uint8_t *d_dist = (uint8_t *)(d_qcnt + FZ_NQ * FZ_CSTRIDE);
	uint64_t *d_peq = carve<uint64_t>(p, (size_t)n_tok * 256);
	uint2 *d_tokf = carve<uint2>(p, (size_t)n_tok + 4);
	uint32_t *d_segoff = carve<uint32_t>(p, (size_t)n_tok + 1);
	uint32_t *d_fill = carve<uint32_t>(p, n_tok);
	uint8_t *d_upb = carve<uint8_t>(p, up_bytes + blen + 16);
	uint32_t *d_up = (uint32_t *)d_upb;
	uint8_t *d_bytes = d_upb + up_bytes;
	uint32_t *d_off = d_up, *d_rank = d_up + n_tok + 1, *d_len_off = d_rank + n_tok;
	fz_args_t fa;

	for (uint32_t i = 0; i <= n_tok; i++) {
		roff[i] = tok_off[i] - tok_off[0];
	}
	for (uint32_t l = 0; l <= NXS_MYERS_MAXPAT + 1; l++) {
		len_off[l] = 0;
	}
	for (uint32_t i = 0; i < n_tok; i++) {
		len_off[roff[i + 1] - roff[i] + 1]++;		/* (every token is <= 64 bytes here) */
	}
	for (uint32_t l = 0; l <= NXS_MYERS_MAXPAT; l++) {
		len_off[l + 1] += len_off[l];
	}
	{
		uint32_t next[NXS_MYERS_MAXPAT + 2];
		memcpy(next, len_off, sizeof(next));
		for (uint32_t i = 0; i < n_tok; i++) {
			rank[i] = next[roff[i + 1] - roff[i]]++;
		}
	}
	memcpy(sd->pin + up_bytes, tok_bytes + tok_off[0], blen);
	if (hipMemcpyAsync(d_upb, sd->pin, up_bytes + blen, hipMemcpyHostToDevice, st) != hipSuccess ||
	    hipMemsetAsync(d_dn, 0, dn_bytes, st) != hipSuccess ||
	    hipMemsetAsync(d_tokf + n_tok, 0xff, 4 * sizeof(uint2), st) != hipSuccess) {
		set_error("suggest upload failed");
		return -1;
	}
	if (prof) (void)hipEventRecord(sd->ev[0], st);
	hipLaunchKernelGGL(k_bk_peq, dim3(n_tok), dim3(256), 0, st, d_bytes, d_off, n_tok, d_peq, d_tokf, d_rank);
	hipLaunchKernelGGL(k_fz_filter, dim3((n_c + 255) / 256, gy), dim3(256), 0, st,
	    sg->d_sig, sg->d_node, sg->d_len, n_c, d_tokf, d_len_off, d_cand, d_qcnt, (uint32_t)qcap, d_cnt + 2);
	if (prof) (void)hipEventRecord(sd->ev[1], st);
	memset(&fa, 0, sizeof(fa));
	fa.bk = ix->d_bk;
	fa.bk_bytes = ix->d_bk_bytes;
	fa.tok_bytes = d_bytes;
	fa.tok_off = d_off;
	fa.peq = d_peq;
	fa.cap = (uint32_t)ccap;
	fa.overflow = d_cnt + 2;
	hipLaunchKernelGGL(k_sg_dist, dim3(8, FZ_NQ), dim3(1024), 0, st, fa, d_cand, d_qcnt, (uint32_t)qcap, maxdist,
	    d_matches, d_match, d_cnt + 1, (uint32_t)mcap);
	if (prof) (void)hipEventRecord(sd->ev[2], st);
	hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(1024), 0, st, d_matches, n_tok, d_segoff, d_fill);
	hipLaunchKernelGGL(k_sg_scatter, dim3(512), dim3(256), 0, st, ix->d_bk, ix->d_post_off, ix->n_terms,
	    d_match, d_cnt + 1, (uint32_t)mcap, d_segoff, d_fill, d_keys);
	if (prof) (void)hipEventRecord(sd->ev[3], st);
	hipLaunchKernelGGL(k_sg_select, dim3(n_tok), dim3(64), 0, st, d_keys, d_segoff, (uint32_t)mcap, k, d_ids, d_dist, d_df, d_counts);
	if (prof) (void)hipEventRecord(sd->ev[4], st);
	if (hipGetLastError() != hipSuccess) {
		set_error("suggest kernel launch failed");
		(void)hipStreamSynchronize(st);
		return -1;
	}
	/* (an overflowed pass: k_sg_scatter and k_sg_select stay inside the arrays -- they check against mcap --
	 * and the rows are thrown away below) */
	if (hipMemcpyAsync(h_dn, d_dn, dn_bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess) {
		set_error("suggest pass failed: %s", hipGetErrorString(hipGetLastError()));
		return -1;
	}
	const uint32_t *h_ids = (const uint32_t *)h_dn, *h_df = h_ids + rows, *h_counts = h_df + rows, *h_matches = h_counts + n_tok;
	const uint32_t *h_cnt = h_matches + n_tok, *h_qcnt = h_cnt + 4;
	const uint8_t *h_dist = (const uint8_t *)(h_qcnt + FZ_NQ * FZ_CSTRIDE);
	if (prof) {
		sg->prof[0] += 1;
		sg->prof[1] += side_elapsed(sd, 0, 4);
		for (int i = 0; i < 4; i++) {
			sg->prof[2 + i] += side_elapsed(sd, i, i + 1);
		}
	}
	if (h_cnt[2]) {
		sg->prof[9] += 1;
		return 1;
	}
	if (prof) {
		for (uint32_t q = 0; q < FZ_NQ; q++) {
			sg->prof[6] += h_qcnt[q * FZ_CSTRIDE];
		}
		sg->prof[7] += h_cnt[1];
	}
	for (uint32_t i = 0; i < n_tok; i++) {
		const size_t to = (size_t)dest[i] * k, from = (size_t)i * k;
		memcpy(o_ids + to, h_ids + from, (size_t)k * 4);
		memcpy(o_df + to, h_df + from, (size_t)k * 4);
		memcpy(o_dist + to, h_dist + from, k);
		o_counts[dest[i]] = h_counts[i];
		o_matches[dest[i]] = h_matches[i];
	}
	return 0;
}

extern "C" int
nxsgpu_suggest(nxsgpu_index_t *ix, const uint8_t *tok_bytes, const uint32_t *tok_off, uint32_t n_tok,
    uint32_t maxdist, uint32_t k, uint32_t *term_ids, uint8_t *dist, uint32_t *df, uint32_t *counts,
    uint32_t *matches)
{
	if (k < 1 || k > NXS_SUGGEST_MAX || maxdist < 1 || maxdist > 2) {
		set_error("nxsgpu_suggest: k is 1..%d, maxdist 1 or 2", NXS_SUGGEST_MAX);
		return -1;
	}
	if (n_tok == 0) {
		return 0;
	}
	if (hipSetDevice(ix->device) != hipSuccess) {
		set_error("hipSetDevice failed");
		return -1;
	}
	if (sg_prepare(ix) != 0) {
		return -1;
	}
	sg_state_t *sg = ix->sg;
	std::vector<uint32_t> dest, off;
	std::vector<uint8_t> bytes;

	memset(term_ids, 0, (size_t)n_tok * k * 4);
	memset(df, 0, (size_t)n_tok * k * 4);
	memset(dist, 0, (size_t)n_tok * k);
	memset(counts, 0, (size_t)n_tok * 4);
	memset(matches, 0, (size_t)n_tok * 4);
	off.push_back(0);
	for (uint32_t i = 0; i < n_tok; i++) {
		const uint32_t m = tok_off[i + 1] - tok_off[i];
		if (ix->cfg.suggest_host || m > NXS_MYERS_MAXPAT) {
#if !defined(__HIP_DEVICE_COMPILE__)	/* (nxs_lev.h keeps its host functions out of the device pass) */
			nxs_suggest_rank(sg->dict.h_terms.data(), sg->dict.h_lens.data(), sg->dict.h_dfs.data(),
			    sg->dict.h_ids.data(), sg->dict.h_terms.size(), tok_bytes + tok_off[i], m, maxdist, k, term_ids + (size_t)i * k,
			    dist + (size_t)i * k, df + (size_t)i * k, &counts[i], &matches[i]);
#endif
			sg->prof[8] += 1;
			continue;
		}
		dest.push_back(i);
		bytes.insert(bytes.end(), tok_bytes + tok_off[i], tok_bytes + tok_off[i + 1]);
		off.push_back((uint32_t)bytes.size());
	}
	const uint32_t nd = (uint32_t)dest.size();
	if (!nd || !sg->n_c) {
		return 0;
	}
	bytes.resize(bytes.size() + 16);
	uint32_t chunk = std::min<uint32_t>(nd, 1u << 20);
	bool full = false;
	for (uint32_t c0 = 0; c0 < nd; ) {
		const uint32_t nc = std::min(chunk, nd - c0);
		const int r = sg_pass(ix, bytes.data(), off.data() + c0, nc, full, maxdist, k, dest.data() + c0,
		    term_ids, dist, df, counts, matches);
		if (r < 0) {
			return -1;
		}
		if (r == 1) {
			/* never a wrong answer: the same tokens again, fewer at a time; one token alone gets
			 * queues that hold whatever the screen can emit */
			if (nc > 1) {
				chunk = std::max<uint32_t>(1, nc / 4);
			} else if (!full) {
				full = true;
			} else {
				set_error("suggest queue overflow (internal error)");
				return -1;
			}
			continue;
		}
		full = false;
		c0 += nc;
	}
	return 0;
}

extern "C" void
nxsgpu_suggest_profile(nxsgpu_index_t *ix, double out[NXSGPU_SUGGEST_PROF], int reset)
{
	memset(out, 0, sizeof(double) * NXSGPU_SUGGEST_PROF);
	if (ix->sg) {
		memcpy(out, ix->sg->prof, sizeof(ix->sg->prof));
		if (reset) {
			memset(ix->sg->prof, 0, sizeof(ix->sg->prof));
		}
	}
}

#ifdef NXS_TEST_HOOKS
/*
 * The device half of nxs_test_term_image (nxs_hooks.h): one part of the term-side state, read back for the test
 * that compares it with a host model (tests/test_term_image.py) -- the BK image, the side arrays and candidates of
 * the match-first search, suggest's candidates, and (through px_test_image) the order that completion and wildcard
 * matching read.  The rules are nxsgpu_test_index_image's: *need = the part's bytes (0: not materialised), copied
 * to `out` if cap holds them; the index's streams and the two states' streams are waited for, device arrays come
 * back by plain hipMemcpy, and NOTHING is built: a state whose generation is behind comes back as it is, which is
 * what the scalars are for.  The part numbers and the scalars' order are restated in nxsearch_amd/__init__.py
 * (TIMG_*).
 */
extern "C" int
nxsgpu_test_term_image(nxsgpu_index_t *ix, int part, void *out, size_t cap, size_t *need)
{
	enum { P_SCALARS, P_BK, P_BK_BYTES, P_BK_PARENT, P_BK_SLOT, P_FZ_NODE, P_FZ_SIG, P_FZ_LEN, P_FZ_LEN_START,
	    P_SG_NODE, P_SG_SIG, P_SG_LEN, P_PX_NODE, P_PX_KEY, P_COUNT };
	const sg_state_t *sg = ix->sg;
	const uint32_t *px_node = NULL;
	const uint64_t *px_key = NULL;
	const void *src = NULL;		/* host memory, or (dev) device memory */
	bool dev = true;
	size_t len = 0;
	uint64_t sc[16] = { 0 }, pxs[4];

	*need = 0;
	if (part < 0 || part >= P_COUNT) {
		set_error("nxsgpu_test_term_image: no part %d", part);
		return -1;
	}
	if (test_image_enter(ix, "nxsgpu_test_term_image") != 0) {
		return -1;
	}
	if (sg && sg->side.st && hipStreamSynchronize(sg->side.st) != hipSuccess) {
		set_error("nxsgpu_test_term_image: hipStreamSynchronize failed");
		return -1;
	}
	if (px_test_image(ix, pxs, &px_node, &px_key) != 0) {
		return -1;
	}
	/* (the side arrays exist with the image or not at all: bk_aux_build) */
	const bool aux = ix->n_bk && ix->d_bk_parent;
	const size_t n_fz = aux ? ix->n_fz : 0, n_sg = sg && sg->built ? sg->n_c : 0, n_px = pxs[0] ? pxs[2] : 0;

	switch (part) {
	case P_SCALARS:
		sc[0] = ix->n_bk;
		sc[1] = ix->bk_depth;
		sc[2] = ix->bk_bytes_len;
		sc[3] = ix->n_fz;
		sc[4] = ix->sg_gen;
		sc[5] = sg ? sg->built : 0;
		sc[6] = sg ? sg->built_gen : 0;
		sc[7] = sg ? sg->n_c : 0;
		sc[8] = ix->px_gen;
		sc[9] = pxs[0];
		sc[10] = pxs[1];
		sc[11] = pxs[2];
		sc[12] = pxs[3];
		src = sc;
		len = sizeof(sc);
		dev = false;
		break;
	case P_BK:
		src = ix->d_bk;
		len = (size_t)ix->n_bk * sizeof(nxsgpu_bknode_t);
		break;
	case P_BK_BYTES:
		src = ix->d_bk_bytes;
		len = ix->n_bk ? ix->bk_bytes_len : 0;
		break;
	case P_BK_PARENT:
		src = ix->d_bk_parent;
		len = aux ? (size_t)ix->n_bk * 4 : 0;
		break;
	case P_BK_SLOT:
		src = ix->d_bk_slot;
		len = aux ? (size_t)ix->n_bk : 0;
		break;
	case P_FZ_NODE:
		src = ix->d_fz_node;
		len = n_fz * 4;
		break;
	case P_FZ_SIG:
		src = ix->d_fz_sig;
		len = n_fz * 4;
		break;
	case P_FZ_LEN:
		src = ix->d_fz_len;
		len = n_fz;
		break;
	case P_FZ_LEN_START:
		src = ix->fz_len_start.data();
		len = aux ? ix->fz_len_start.size() * 4 : 0;
		dev = false;
		break;
	case P_SG_NODE:
		src = sg ? sg->d_node : NULL;
		len = n_sg * 4;
		break;
	case P_SG_SIG:
		src = sg ? sg->d_sig : NULL;
		len = n_sg * 4;
		break;
	case P_SG_LEN:
		src = sg ? sg->d_len : NULL;
		len = n_sg;
		break;
	case P_PX_NODE:
		src = px_node;
		len = n_px * 4;
		break;
	case P_PX_KEY:
		src = px_key;
		len = n_px * 8;
		break;
	}
	if (!src) {
		len = 0;
	}
	*need = len;
	if (!len || !out || cap < len) {
		return 0;
	}
	if (!dev) {
		memcpy(out, src, len);
	} else if (hipMemcpy(out, src, len, hipMemcpyDeviceToHost) != hipSuccess) {
		set_error("nxsgpu_test_term_image: hipMemcpy of part %d failed", part);
		return -1;
	}
	return 0;
}
#endif /* NXS_TEST_HOOKS */
