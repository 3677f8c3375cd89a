/*
 * nxs_complete.h -- the host ranker of prefix completions, shared by the C11 host
 * code (the test hook) and the host side of the HIP shim (nxsgpu_complete under
 * NXS_GPU_COMPLETE=host).
 *
 * Plain and exact, not fast: a linear scan over the dictionary.  A term is
 * eligible when its df is > 0 and its first `len` bytes equal the prefix (the
 * term equal to the prefix included); the best k by (df descending, term id
 * ascending) are kept in a sorted array.  This is the definition the device
 * pass (nxs_gpu_prefix.hip) is checked against.
 */
#ifndef NXS_COMPLETE_H
#define NXS_COMPLETE_H

#include <stdint.h>
#include <stddef.h>
#include <string.h>

#define	NXS_COMPLETE_MAX	32	/* (= NXS_SUGGEST_MAX, include/nxs.h) */

/* does (df1, id1) come before (df2, id2)? */
static inline int
nxs_complete_before(uint32_t df1, uint32_t id1, uint32_t df2, uint32_t id2)
{
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
nxs_complete_rank(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs, const uint32_t *ids,
    size_t n, const uint8_t *prefix, size_t len, uint32_t k,
    uint32_t *out_ids, uint32_t *out_df, uint32_t *count, uint32_t *matches)
{
	uint32_t have = 0, total = 0;

	for (size_t i = 0; i < n; i++) {
		const uint32_t id = ids ? ids[i] : (uint32_t)i + 1;
		uint32_t at;

		if (!dfs[i] || lens[i] < len || (len && memcmp(terms[i], prefix, len) != 0)) {
			continue;
		}
		total++;
		if (have == k && !nxs_complete_before(dfs[i], id, out_df[k - 1], out_ids[k - 1])) {
			continue;
		}
		at = have < k ? have++ : k - 1;
		while (at > 0 && nxs_complete_before(dfs[i], id, out_df[at - 1], out_ids[at - 1])) {
			out_ids[at] = out_ids[at - 1];
			out_df[at] = out_df[at - 1];
			at--;
		}
		out_ids[at] = id;
		out_df[at] = dfs[i];
	}
	*count = have;
	*matches = total;
}

#endif
