/*
 * nxs_wild.h -- wildcard patterns over dictionary terms, shared by the C11 host code and the HIP side
 * (compiled by both gcc and hipcc): the matcher that the device kernel (k_wc_match, nxs_gpu_wild.hip) and
 * the host run alike, and the plain host ranker the device pass is checked against (the route of
 * nxsgpu_wildcard under NXS_GPU_WILDCARD=host).
 *
 * A pattern is a byte string: `*` matches any run of bytes (the empty one included), `?` exactly one byte,
 * every other byte itself; no escapes, no classes.  A term matches when the whole term matches the whole
 * pattern.  Byte-wise, as the Levenshtein distance and the prefixes are.
 */
#ifndef NXS_WILD_H
#define NXS_WILD_H

#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define	NXS_WILD_HD	__host__ __device__ static inline
#else
#define	NXS_WILD_HD	static inline
#endif

#ifndef NXS_WILD_MAXLEN
#define	NXS_WILD_MAXLEN		255	/* bytes of a normalised pattern at most (include/nxs.h) */
#endif
#define	NXS_WILD_MAX		32	/* terms a call or a leaf takes at most (= NXS_SUGGEST_MAX, include/nxs.h) */
#define	NXS_WILD_INL		8	/* a BK node carries this many leading bytes of its term (nxsgpu_bknode_t::inl) */

NXS_WILD_HD int
nxs_wild_meta(uint8_t c)
{
	return c == '*' || c == '?';
}

/* the literal head: the bytes before the first metacharacter */
NXS_WILD_HD uint32_t
nxs_wild_head(const uint8_t *pat, uint32_t plen)
{
	uint32_t h = 0;

	while (h < plen && !nxs_wild_meta(pat[h])) {
		h++;
	}
	return h;
}

/* *literals = the bytes that are no metacharacter, *minlen = the bytes that are no star (the shortest term
 * that can match; without a star the only length that can) -> is there a star? */
NXS_WILD_HD int
nxs_wild_shape(const uint8_t *pat, uint32_t plen, uint32_t *literals, uint32_t *minlen)
{
	uint32_t lit = 0, stars = 0;

	for (uint32_t i = 0; i < plen; i++) {
		lit += !nxs_wild_meta(pat[i]);
		stars += pat[i] == '*';
	}
	*literals = lit;
	*minlen = plen - stars;
	return stars != 0;
}

/*
 * The matcher proper, two cursors: t walks the term, p the pattern; the last star met and the term position
 * it was tried at are remembered, and a mismatch behind it lets that star take one byte more.  No
 * recursion, no allocation; every restart moves `mark` forward and a run between restarts is at most plen
 * steps, so the cost is O(tlen x plen) at worst (`*a*a*a*b` against a run of `a`: a product, not an
 * exponent).  Lengths are 32-bit: terms of the 65535 bytes a str_len carries are fine.
 *
 * Term byte j is inl >> 8 j for j < n_inl (the node's inline bytes, loaded as one little-endian word: a
 * lane keeps them in a register pair) and bytes[j] from there on; the host passes n_inl = 0.
 */
NXS_WILD_HD int
nxs_wild_match_inl(uint64_t inl, uint32_t n_inl, const uint8_t *bytes, uint32_t tlen,
    const uint8_t *pat, uint32_t plen)
{
	const uint32_t none = ~(uint32_t)0;
	uint32_t t = 0, p = 0, star = none, mark = 0;

	while (t < tlen) {
		const uint8_t c = t < n_inl ? (uint8_t)(inl >> (8 * t)) : bytes[t];

		if (p < plen && pat[p] == '*') {
			star = p++;
			mark = t;
		} else if (p < plen && (pat[p] == '?' || pat[p] == c)) {
			p++;
			t++;
		} else if (star != none) {
			p = star + 1;
			t = ++mark;
		} else {
			return 0;
		}
	}
	while (p < plen && pat[p] == '*') {
		p++;
	}
	return p == plen;
}

NXS_WILD_HD int
nxs_wild_match(const uint8_t *term, size_t tlen, const uint8_t *pat, size_t plen)
{
	return nxs_wild_match_inl(0, 0, term, (uint32_t)tlen, pat, (uint32_t)plen);
}

/* does (df1, id1) come before (df2, id2)?  df descending, then term id ascending */
static inline int
nxs_wild_before(uint32_t df1, uint32_t id1, uint32_t df2, uint32_t id2)
{
	if (df1 != df2) {
		return df1 > df2;
	}
	return id1 < id2;
}

/*
 * The host ranker: plain and exact, not fast -- a linear scan over the dictionary, the best k kept in a
 * sorted array.  terms[i] / lens[i] / dfs[i]: the dictionary, n entries; ids[i] their term ids (NULL:
 * i + 1).  A term is eligible when its df is > 0 and it matches.  out_*: room for k entries.
 * *count = min(k, *matches).
 */
static inline void
nxs_wild_rank(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs, const uint32_t *ids,
    size_t n, const uint8_t *pat, size_t plen, uint32_t k,
    uint32_t *out_ids, uint32_t *out_df, uint32_t *count, uint32_t *matches)
{
	uint32_t have = 0, total = 0;

	for (size_t i = 0; i < n; i++) {
		const uint32_t id = ids ? ids[i] : (uint32_t)i + 1;
		uint32_t at;

		if (!dfs[i] || !nxs_wild_match(terms[i], lens[i], pat, plen)) {
			continue;
		}
		total++;
		if (have == k && !nxs_wild_before(dfs[i], id, out_df[k - 1], out_ids[k - 1])) {
			continue;
		}
		at = have < k ? have++ : k - 1;
		while (at > 0 && nxs_wild_before(dfs[i], id, out_df[at - 1], out_ids[at - 1])) {
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
