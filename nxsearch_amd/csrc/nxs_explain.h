/*
 * nxs_explain.h -- the searches behind an explanation (nxsgpu_explain), shared by the HIP kernel
 * and the C11 host code (compiled by both hipcc and gcc; the CPU tier tests them through a hook).
 *
 * An explanation cell is a (result doc, query token) pair: is there a posting of the token's term in
 * the doc, and where.  Three searches answer it:
 *
 *   nxs_ex_ordinal   the doc id's ordinal: a lower bound over the ascending (possibly sparse, u64)
 *                    ids of the live docs;
 *   nxs_ex_lower     a lower bound over a run of the term's list -- entries doc << 32 | tf, ascending
 *                    by doc.  Branch-free: the trip count follows from the run's length alone, so all
 *                    lanes of a wavefront that search the same list take the same steps, and their
 *                    first probes fall into the same cache lines;
 *   nxs_ex_find      the lookup itself.  A term with a block-presence bitmap answers "absent" from
 *                    the doc's 64-doc block bit (one load) and else searches only the span of the
 *                    doc's 4096-doc word, which the rank directory delimits; a term without one
 *                    searches its whole list.
 */
#ifndef NXS_EXPLAIN_H
#define NXS_EXPLAIN_H

#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define	NXS_EX_HD	__host__ __device__ static inline
#else
#define	NXS_EX_HD	static inline
#endif

#define	NXS_EX_NONE	UINT64_MAX

/* the ordinal of doc id `id` in ids[0 .. n) (ascending, distinct), or NXS_EX_NONE */
NXS_EX_HD uint64_t
nxs_ex_ordinal(const uint64_t *ids, uint64_t n, uint64_t id)
{
	uint64_t base = 0;

	if (n == 0) {
		return NXS_EX_NONE;
	}
	while (n > 1) {
		const uint64_t half = n >> 1;
		base = ids[base + half - 1] < id ? base + half : base;
		n -= half;
	}
	return ids[base] == id ? base : NXS_EX_NONE;
}

/* first position p in [lo, hi) with (dt[p] >> 32) >= doc, hi if there is none */
NXS_EX_HD uint64_t
nxs_ex_lower(const uint64_t *dt, uint64_t lo, uint64_t hi, uint32_t doc)
{
	uint64_t base = lo, n = hi - lo;

	if (n == 0) {
		return hi;
	}
	while (n > 1) {
		const uint64_t half = n >> 1;
		base = (uint32_t)(dt[base + half - 1] >> 32) < doc ? base + half : base;
		n -= half;
	}
	return base + ((uint32_t)(dt[base] >> 32) < doc ? 1 : 0);
}

/*
 * The posting of doc ordinal `doc` in the list dt[beg .. end): its position, or NXS_EX_NONE.
 * blkmap / bmrank: the term's rows of the block-presence bitmap ([words], one bit per 64-doc block)
 * and of its rank directory ([words + 1], list-relative position of the first posting at or above
 * each 4096-doc word), or both NULL.
 */
NXS_EX_HD uint64_t
nxs_ex_find(const uint64_t *dt, uint64_t beg, uint64_t end, const uint64_t *blkmap, const uint32_t *bmrank,
    uint32_t doc)
{
	uint64_t lo = beg, hi = end, p;

	if (blkmap) {
		const uint32_t w = doc >> 12;

		if (!((blkmap[w] >> ((doc >> 6) & 63)) & 1)) {
			return NXS_EX_NONE;
		}
		lo = beg + bmrank[w];
		hi = beg + bmrank[w + 1];
	}
	p = nxs_ex_lower(dt, lo, hi, doc);
	return (p < hi && (uint32_t)(dt[p] >> 32) == doc) ? p : NXS_EX_NONE;
}

#endif /* NXS_EXPLAIN_H */
