/*
 * nxs_docterms.h -- the lookups behind a doc's term vector (nxsgpu_doc_terms), shared by the HIP kernels and
 * the C11 host code (compiled by both hipcc and gcc; the CPU tier tests them through a hook), beside
 * nxs_explain.h, whose searches they rest on.
 *
 * There is no forward index: a doc's terms are found by asking every term's list for the doc.  A CHUNK is at
 * most 64 docs of a batch as ascending, distinct ordinals; one list is matched against a chunk from the
 * shorter side:
 *
 *   by doc       nxs_ex_find per ordinal: the block bit where the term has a bitmap row, a branch-free lower
 *                bound over the span the rank directory delimits (or the whole list) else;
 *   by posting   for a list shorter than the chunk and without a bitmap row: one lower bound per posting
 *                over the chunk's ordinals (nxs_dv_slot).
 *
 *   nxs_dv_key   the selection key of an eligible (term, doc): the impact's bits complemented above the term
 *                id, so that ascending keys are impact descending, term id ascending.  Keys of one doc are
 *                distinct.  (Eligible means w >= 0: the bits of non-negative floats order as the floats do;
 *                -0.0 equals 0.0 as a float and takes its key.)
 *   nxs_dv_term  one list against one chunk, either way: the position of every chunk doc's posting.
 */
#ifndef NXS_DOCTERMS_H
#define NXS_DOCTERMS_H

#include <string.h>

#include "nxs_explain.h"

#define	NXS_DV_CHUNK	64		/* docs per chunk at most */
#define	NXS_DV_NOSLOT	0xffffffffu

/* the slot of ordinal `doc` in ords[0 .. nd) (ascending, distinct; nd >= 1), or NXS_DV_NOSLOT */
NXS_EX_HD uint32_t
nxs_dv_slot(const uint32_t *ords, uint32_t nd, uint32_t doc)
{
	uint32_t base = 0, n = nd;

	while (n > 1) {
		const uint32_t half = n >> 1;
		base = ords[base + half - 1] < doc ? base + half : base;
		n -= half;
	}
	return ords[base] == doc ? base : NXS_DV_NOSLOT;
}

/* is a list of `len` postings matched by posting against a chunk of nd docs? */
NXS_EX_HD bool
nxs_dv_by_posting(uint64_t len, uint32_t nd, bool has_bitmap)
{
	return !has_bitmap && len < nd;
}

NXS_EX_HD uint64_t
nxs_dv_key(float w, uint32_t term)
{
	uint32_t bits;

	if (w == 0.0f) {
		w = 0.0f;
	}
	memcpy(&bits, &w, 4);
	return (uint64_t)~bits << 32 | term;
}

/*
 * The list dt[beg .. end) against the chunk ords[0 .. nd): pos[j] = the position of ordinal j's posting, or
 * NXS_EX_NONE.  by_posting selects the side the searches start from (blkmap / bmrank are read by doc only).
 */
NXS_EX_HD void
nxs_dv_term(const uint64_t *dt, uint64_t beg, uint64_t end, const uint64_t *blkmap, const uint32_t *bmrank,
    const uint32_t *ords, uint32_t nd, bool by_posting, uint64_t *pos)
{
	for (uint32_t j = 0; j < nd; j++) {
		pos[j] = by_posting ? NXS_EX_NONE : nxs_ex_find(dt, beg, end, blkmap, bmrank, ords[j]);
	}
	for (uint64_t p = beg; by_posting && nd && p < end; p++) {
		const uint32_t j = nxs_dv_slot(ords, nd, (uint32_t)(dt[p] >> 32));

		if (j != NXS_DV_NOSLOT) {
			pos[j] = p;
		}
	}
}

#endif /* NXS_DOCTERMS_H */
