/*
 * nxs_related.h -- the order of related terms (nxsgpu_related), shared by the HIP kernels and the C11 host code
 * (compiled by both hipcc and gcc; the CPU tier tests it through a hook), beside nxs_docterms.h, whose key it
 * rests on.
 *
 * For a doc set M and a dictionary term t: c = the docs of M that hold t, df = the live df (the length of t's
 * list).
 *
 *   nxs_rt_share     s = the f32 nearest to the fp64 quotient (double)c / (double)df.  IEEE division and one
 *                    rounding to f32: no contraction, no reciprocal (the units are built with -ffp-contract=off).
 *   nxs_rt_key       the selection key of (c, df, t): ascending keys are the order.  NXS_RT_COUNT: ~c above the
 *                    term id (c descending, term id ascending).  NXS_RT_SHARE: nxs_dv_key(s, t) as it stands
 *                    (s >= 0: the bits of non-negative floats order as the floats do).  Keys of one query are
 *                    distinct, and none is 0 or ~0.
 *   nxs_rt_eligible  c >= mincount, df >= mindf, and t is not among the n_excl excluded term ids (the query's
 *                    resolved token list; n_excl = 0 under "related_self").
 *   nxs_rt_rank      the host ranker: every eligible term's key, a plain sort, the first k.
 */
#ifndef NXS_RELATED_H
#define NXS_RELATED_H

#include <stdlib.h>

#include "nxs_docterms.h"

enum { NXS_RT_COUNT = 0, NXS_RT_SHARE = 1 };

#define	NXS_RT_EXCL_MAX	32		/* excluded term ids at most: the tokens of a fixed-size plan */

NXS_EX_HD float
nxs_rt_share(uint32_t c, uint32_t df)
{
	return (float)((double)c / (double)df);
}

NXS_EX_HD uint64_t
nxs_rt_key(int order, uint32_t c, uint32_t df, uint32_t term)
{
	if (order == NXS_RT_SHARE) {
		return nxs_dv_key(nxs_rt_share(c, df), term);
	}
	return (uint64_t)~c << 32 | term;
}

NXS_EX_HD bool
nxs_rt_eligible(uint32_t c, uint32_t df, uint32_t mincount, uint32_t mindf, uint32_t term, const uint32_t *excl,
    uint32_t n_excl)
{
	if (c < mincount || df < mindf || df == 0) {
		return false;
	}
	for (uint32_t i = 0; i < n_excl; i++) {
		if (excl[i] == term) {
			return false;
		}
	}
	return true;
}

/* (host only from here on) */
static inline int
nxs_rt_key_cmp(const void *a, const void *b)
{
	const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;

	return x < y ? -1 : x > y;
}

/*
 * c[t], df[t] for the term ids t = 1 .. n_terms (slot 0 is not read).  out_ids[0 .. k): the first
 * min(k, *matches) eligible terms in the order; *matches: how many are eligible.  -> how many were written,
 * -1: out of memory.
 */
static inline int
nxs_rt_rank(int order, const uint32_t *c, const uint32_t *df, uint32_t n_terms, uint32_t mincount, uint32_t mindf,
    const uint32_t *excl, uint32_t n_excl, uint32_t k, uint32_t *out_ids, uint64_t *matches)
{
	uint64_t *keys, n = 0;
	uint32_t m = 0;

	*matches = 0;
	for (uint32_t t = 1; t <= n_terms; t++) {
		m += c[t] >= mincount && c[t] != 0;	/* (an upper bound of the eligible terms: the array's size) */
	}
	if ((keys = (uint64_t *)malloc(((size_t)m + 1) * sizeof(*keys))) == NULL) {
		return -1;
	}
	for (uint32_t t = 1; t <= n_terms; t++) {
		if (c[t] != 0 && nxs_rt_eligible(c[t], df[t], mincount, mindf, t, excl, n_excl)) {
			keys[n++] = nxs_rt_key(order, c[t], df[t], t);
		}
	}
	qsort(keys, n, sizeof(*keys), nxs_rt_key_cmp);
	*matches = n;
	m = n < k ? (uint32_t)n : k;
	for (uint32_t r = 0; r < m; r++) {
		out_ids[r] = (uint32_t)keys[r];
	}
	free(keys);
	return (int)m;
}

#endif /* NXS_RELATED_H */
