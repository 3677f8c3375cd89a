/*
 * nxs_docset.h -- a search within a caller's doc-id set (nxsgpu_search_docs), shared by the HIP kernels and the C11
 * host code (compiled by both hipcc and gcc; the CPU tier tests it through hooks), on top of nxs_explain.h's
 * searches.
 *
 * The scoring is driven from the DOCS, not from the lists: for a doc ordinal and a query's token table every
 * token's list is asked for the doc (nxs_ex_find), which gives the presence mask the expression is evaluated on
 * and the floats run_query_logic would add (search.c:236-270).
 *
 *   nxs_ds_sort_unique  a set as the device wants it: ascending, distinct u64 ids.  One pass detects input that is
 *                       already so and skips the sort.
 *   nxs_ds_prog_ok      is a postfix program one the evaluators handle (operands, underflow, depth <= 64)
 *   nxs_ds_eval         the postfix program of a fixed-size plan on a presence mask (a bit stack: such a plan's
 *                       evaluation stack is at most 64 deep).  Host + device: the related pass's host route
 *                       evaluates its doc sets with it too.
 *   nxs_ds_lane         one doc ordinal against a token table: is the doc a result, and with what score.  For each
 *                       token the float is d_post[algo] at the position of the doc's posting in the primary CSR --
 *                       the REGULAR posting of a TF-IDF dense term, never its outlier list, as nxsgpu_explain reads
 *                       it.  A result: the expression holds on the presence mask (truth table up to 8 tokens, the
 *                       program above that) and at least one present token has a non-negative float
 *                       (search.c:251-258).  The score is the f32 sum of the non-negative floats in ascending token
 *                       order, starting from 0 (a term listed twice adds twice).
 */
#ifndef NXS_DOCSET_H
#define NXS_DOCSET_H

#include <stdbool.h>
#include <stdlib.h>

#include "nxs_gpu.h"
#include "nxs_explain.h"

#define	NXS_DS_NONE	0xffffffffu	/* a set entry that is not in the doc table; a token without a bitmap row */

/* one token of one query: its list in the CSR and its bitmap row (NXS_DS_NONE: none) */
typedef struct {
	uint64_t	beg, end;
	uint32_t	row, pad;
} nxs_ds_tok_t;

/* a posting of d_post[algo] (posting_t, nxs_gpu_int.h) as C sees it */
typedef struct {
	uint32_t	doc;
	float		imp;
} nxs_ds_post_t;

/*
 * Is prog[0 .. len) a program nxs_ds_eval (and the kernels' eval_prog) evaluates as written: every push names a token
 * below nt or the empty set, no operator finds fewer than two values, the stack never holds more than 64, and one
 * value at least is left.  What nxs_query.c compiles always is; the C-ABI entry points check a plan they are handed.
 */
NXS_EX_HD bool
nxs_ds_prog_ok(const uint8_t *prog, uint32_t len, uint32_t nt)
{
	uint32_t depth = 0;

	for (uint32_t i = 0; i < len; i++) {
		const uint8_t op = prog[i];

		if (op < NXSGPU_MAX_TOKENS || op == NXSGPU_OP_EMPTY) {
			if ((op != NXSGPU_OP_EMPTY && op >= nt) || ++depth > 64) {
				return false;
			}
		} else if ((op != NXSGPU_OP_AND && op != NXSGPU_OP_OR && op != NXSGPU_OP_ANDNOT) || depth < 2) {
			return false;
		} else {
			depth--;
		}
	}
	return depth >= 1;
}

/*
 * The evaluator of the doc-driven code (k_ds_score through nxs_ds_lane, and the host routes): the same bit stack as
 * the scan and count kernels' eval_prog (nxs_gpu_dev.h), which is device-only code of a HIP header and cannot be
 * called from a header gcc compiles; the two bodies are to stay line for line alike.  Precondition: nxs_ds_prog_ok.
 */
NXS_EX_HD bool
nxs_ds_eval(const uint8_t *prog, uint32_t len, uint32_t m)
{
	uint64_t st = 0;	/* bit stack, top at bit 0 */

	for (uint32_t i = 0; i < len; i++) {
		const uint8_t op = prog[i];

		if (op < NXSGPU_MAX_TOKENS) {
			st = (st << 1) | ((m >> op) & 1u);
		} else if (op == NXSGPU_OP_EMPTY) {
			st <<= 1;
		} else {
			const uint64_t b = st & 1, a = (st >> 1) & 1;
			const uint64_t r = op == NXSGPU_OP_AND ? (a & b) : op == NXSGPU_OP_OR ? (a | b) : (a & ~b & 1);

			st = ((st >> 2) << 1) | r;
		}
	}
	return st & 1;
}

/*
 * Doc ordinal `ord` against toks[0 .. nt) (nt <= NXSGPU_MAX_TOKENS).  truth: the plan's 256-bit table (read when
 * nt <= 8), prog: its postfix program (read above that).  blkmap / bmrank: the index's bitmap rows and rank
 * directories ([rows][bm_words], [rows][bm_words + 1]).  -> is the doc a result; *score then holds its score.
 */
NXS_EX_HD bool
nxs_ds_lane(uint32_t ord, uint32_t nt, const nxs_ds_tok_t *toks, const uint32_t *truth, const uint8_t *prog,
    uint32_t prog_len, const uint64_t *post_dt, const nxs_ds_post_t *post, const uint64_t *blkmap,
    const uint32_t *bmrank, uint64_t bm_words, float *score)
{
	uint32_t pres = 0;
	bool scored = false;
	float s = 0.0f;

	for (uint32_t j = 0; j < nt; j++) {
		const nxs_ds_tok_t t = toks[j];		/* same address in every lane */

		if (t.beg < t.end) {
			const bool bm = t.row != NXS_DS_NONE;
			const uint64_t p = nxs_ex_find(post_dt, t.beg, t.end,
			    bm ? blkmap + (uint64_t)t.row * bm_words : (const uint64_t *)NULL,
			    bm ? bmrank + (uint64_t)t.row * (bm_words + 1) : (const uint32_t *)NULL, ord);

			if (p != NXS_EX_NONE) {
				const float f = post[p].imp;

				pres |= 1u << j;
				/* search.c:261: a negative rank() adds nothing */
				if (f >= 0.0f) {
					s += f;
					scored = true;
				}
			}
		}
	}
	*score = s;
	if (!scored) {
		return false;
	}
	return nt <= 8 ? (truth[pres >> 5] >> (pres & 31)) & 1u : nxs_ds_eval(prog, prog_len, pres);
}

/* (host only from here on) */
static inline int
nxs_ds_id_cmp(const void *a, const void *b)
{
	const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;

	return x < y ? -1 : x > y;
}

/* ids[0 .. n) in place: ascending, distinct -> how many are left */
static inline size_t
nxs_ds_sort_unique(uint64_t *ids, size_t n)
{
	size_t i, m;

	for (i = 1; i < n && ids[i - 1] < ids[i]; i++) {
		;
	}
	if (i >= n) {
		return n;		/* already ascending and distinct */
	}
	qsort(ids, n, sizeof(*ids), nxs_ds_id_cmp);
	for (i = 1, m = 1; i < n; i++) {
		if (ids[i] != ids[m - 1]) {
			ids[m++] = ids[i];
		}
	}
	return m;
}

#endif /* NXS_DOCSET_H */
