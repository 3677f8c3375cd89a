/*
 * nxs_suggest.h -- the host ranker of spelling suggestions, shared by the C11 host
 * code (the test hook) and the host side of the HIP shim (nxsgpu_suggest: tokens
 * beyond the bit-vector distance, and everything under NXS_GPU_SUGGEST=host).
 *
 * Plain and exact, not fast: every term with df > 0 whose length is within
 * maxdist of the token's takes nxs_levdist_host (nxs_lev.h); the best k by
 * (distance ascending, df descending, term id ascending) are kept in a sorted
 * array.  This is the definition the device pass is checked against.
 */
#ifndef NXS_SUGGEST_H
#define NXS_SUGGEST_H

#include <stdint.h>
#include <stddef.h>

#include "nxs_lev.h"

#define	NXS_SUGGEST_MAX		32	/* (= include/nxs.h) */

#if !defined(__HIPCC__) || !defined(__HIP_DEVICE_COMPILE__)

/* does (d1, df1, id1) come before (d2, df2, id2)? */
static inline int
nxs_suggest_before(uint32_t d1, uint32_t df1, uint32_t id1, uint32_t d2, uint32_t df2, uint32_t id2)
{
	if (d1 != d2) {
		return d1 < d2;
	}
	if (df1 != df2) {
		return df1 > df2;
	}
	return id1 < id2;
}

/*
 * terms[i] / lens[i] / dfs[i]: the dictionary, n entries; ids[i] their term ids
 * (NULL: i + 1).  out_*: room for k entries.  *count = min(k, *matches).
 */
static inline void
nxs_suggest_rank(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs, const uint32_t *ids,
    size_t n, const uint8_t *token, size_t len, uint32_t maxdist, uint32_t k,
    uint32_t *out_ids, uint8_t *out_dist, uint32_t *out_df, uint32_t *count, uint32_t *matches)
{
	uint32_t have = 0, total = 0;

	for (size_t i = 0; i < n; i++) {
		const size_t tl = lens[i];
		const uint32_t id = ids ? ids[i] : (uint32_t)i + 1;
		uint32_t d, at;

		if (!dfs[i] || (tl > len ? tl - len : len - tl) > maxdist) {
			continue;
		}
		d = (uint32_t)nxs_levdist_host(terms[i], tl, token, len);
		if (d > maxdist) {
			continue;
		}
		total++;
		if (have == k && !nxs_suggest_before(d, dfs[i], id, out_dist[k - 1], out_df[k - 1], out_ids[k - 1])) {
			continue;
		}
		at = have < k ? have++ : k - 1;
		while (at > 0 && nxs_suggest_before(d, dfs[i], id, out_dist[at - 1], out_df[at - 1], out_ids[at - 1])) {
			out_ids[at] = out_ids[at - 1];
			out_dist[at] = out_dist[at - 1];
			out_df[at] = out_df[at - 1];
			at--;
		}
		out_ids[at] = id;
		out_dist[at] = (uint8_t)d;
		out_df[at] = dfs[i];
	}
	*count = have;
	*matches = total;
}

#endif
#endif
