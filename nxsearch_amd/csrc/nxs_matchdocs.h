/*
 * nxs_matchdocs.h -- a query's matches listed by doc id (nxsgpu_match_docs), shared by the HIP kernels and the C11
 * host code (compiled by both hipcc and gcc; the CPU tier tests it through a hook, tools/matchdocs_selftest.c runs
 * it stand-alone).
 *
 * A PAGE of a doc set M for a cursor `from` and a limit: the docs of M whose id is >= from, in ascending doc id,
 * the first `limit` of them; `more` = a doc of M lies beyond the page.  Doc ordinals ascend with doc ids, so the
 * cursor becomes an ordinal once (nxs_md_lower_bound) and the page is the first `limit` set bits from there on.
 *
 *   nxs_md_lower_bound  the first ordinal whose doc id is >= from (n if none): k_md_from's lane and the host's
 *   nxs_md_page         the host definition of a page over M as bits per doc ordinal: the cross-check route and
 *                       what the device pass is tested against
 */
#ifndef NXS_MATCHDOCS_H
#define NXS_MATCHDOCS_H

#include <stdbool.h>
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define	NXS_MD_HD	__host__ __device__ static inline
#else
#define	NXS_MD_HD	static inline
#endif

/* the first i in [0, n] with ids[i] >= from (ids ascending; n: every id is below from) */
NXS_MD_HD uint64_t
nxs_md_lower_bound(const uint64_t *ids, uint64_t n, uint64_t from)
{
	uint64_t lo = 0, hi = n;

	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo) >> 1);

		if (ids[mid] < from) {
			lo = mid + 1;
		} else {
			hi = mid;
		}
	}
	return lo;
}

/* (host only from here on) */

/*
 * in_bits: M as bits per doc ordinal, (D + 31) / 32 words, bit (d & 31) of word d >> 5; doc_ids[0 .. D) ascending.
 * out[0 .. min(limit, D)) receives the page; -> how many ids were written, *more = a doc of M lies beyond them.
 */
static inline uint64_t
nxs_md_page(const uint32_t *in_bits, const uint64_t *doc_ids, uint64_t D, uint64_t from, uint64_t limit, uint64_t *out,
    bool *more)
{
	uint64_t n = 0;

	*more = false;
	for (uint64_t d = nxs_md_lower_bound(doc_ids, D, from); d < D; d++) {
		if ((in_bits[d >> 5] >> (d & 31)) & 1u) {
			if (n == limit) {
				*more = true;
				break;
			}
			out[n++] = doc_ids[d];
		}
	}
	return n;
}

#endif /* NXS_MATCHDOCS_H */
