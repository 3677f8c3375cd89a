/*
 * nxs_hooks.c -- the test hooks of nxs_hooks.h that reach no unit's statics:
 * host-only pieces, exercised without a GPU.  (A hook that reaches a static
 * lives in that static's unit.)
 */
#ifdef NXS_TEST_HOOKS
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"
#include "nxs_suggest.h"
#include "nxs_complete.h"
#include "nxs_wild.h"
#include "nxs_explain.h"
#include "nxs_docterms.h"
#include "nxs_related.h"
#include "nxs_docset.h"
#include "nxs_matchdocs.h"

char *
nxs_test_query_repr(const char *query, char **errmsg)
{
	qparse_t q;
	char *r;

	nxs_query_parse(query, &q);
	r = nxs_query_repr(&q);
	if (errmsg) {
		*errmsg = q.errmsg ? strdup(q.errmsg) : NULL;
	}
	nxs_query_free(&q);
	return r;
}

/*
 * Compile a query against a caller-supplied dictionary (words[i] has term id
 * i+1); unknown words stay unresolved.  Writes the plan; returns the error
 * code (0 = ok), *empty = no live tokens.
 */
int
nxs_test_compile(const char *query, const char *const *words, uint32_t n_words,
    bool lowercase, nxsgpu_query_t *plan, int *empty, char *err, size_t errlen)
{
	nxs_index_t fake = { .lowercase = lowercase };
	qprep_t q;
	int code;

	nxs_query_prepare(&fake, query, &q);
	if (!q.errcode) {
		for (size_t j = 0; j < q.n_tokens; j++) {
			for (uint32_t w = 0; w < n_words; w++) {
				if (strlen(words[w]) == q.tokens[j].len &&
				    memcmp(words[w], q.tokens[j].value, q.tokens[j].len) == 0) {
					q.tokens[j].term_id = w + 1;
					break;
				}
			}
		}
		(void)nxs_query_compile(&q);
	}
	code = q.errcode;
	if (err && errlen) {
		snprintf(err, errlen, "%s", q.errmsg ? q.errmsg : "");
	}
	*plan = q.plan;
	*empty = q.empty;
	nxs_query_release(&q);
	return code;
}

/*
 * The same for queries that take the wide plan: *wide = 1 and the plan's
 * arrays are copied out (term_ids[cap_t], prog[cap_p]); returns the error code.
 */
int
nxs_test_compile_wide(const char *query, const char *const *words, uint32_t n_words,
    int *wide, uint32_t *n_tokens, uint32_t *term_ids, uint32_t cap_t,
    uint32_t *prog_len, uint16_t *prog, uint32_t cap_p)
{
	nxs_index_t fake = { .lowercase = false };
	qprep_t q;
	int code;

	nxs_query_prepare(&fake, query, &q);
	if (!q.errcode) {
		for (size_t j = 0; j < q.n_tokens; j++) {
			/* words are "w<id>" here: resolve by number, not by search */
			const char *v = q.tokens[j].value;
			if (v[0] == 'w') {
				const unsigned long id = strtoul(v + 1, NULL, 10);
				if (id >= 1 && id <= n_words && strcmp(words[id - 1], v) == 0) {
					q.tokens[j].term_id = (uint32_t)id;
				}
			}
		}
		(void)nxs_query_compile(&q);
	}
	code = q.errcode;
	*wide = q.wide;
	*n_tokens = q.wide ? q.wplan.n_tokens : q.plan.n_tokens;
	*prog_len = q.wide ? q.wplan.prog_len : q.plan.prog_len;
	if (q.wide && q.wplan.n_tokens <= cap_t && q.wplan.prog_len <= cap_p) {
		memcpy(term_ids, q.wplan.term_id, q.wplan.n_tokens * sizeof(uint32_t));
		memcpy(prog, q.wplan.prog, q.wplan.prog_len * sizeof(uint16_t));
	}
	nxs_query_release(&q);
	return code;
}

/* a pipeline of the normalizer (+ stop words from `basedir`: bit 0 of `stages`, + the English stemmer: bit 1),
 * its stages in `run` on one string -> malloc'd result, NULL if discarded or on error (*act tells which) */
static char *
test_filter(const char *basedir, int stages, unsigned run, const char *s, int *act)
{
	const char *names[3] = { "normalizer" };
	size_t n = 1;
	const char *err = NULL;
	nxs_filters_t *f;
	if (stages & 1) names[n++] = "stopwords";
	if (stages & 2) names[n++] = "stemmer";
	f = nxs_filters_create(basedir, names, n, "en", &err);
	char *val = strdup(s);
	size_t len = strlen(s);

	*act = -2;
	if (!f) {
		free(val);
		return NULL;
	}
	*act = nxs_filters_run_stages(f, run, &val, &len);
	nxs_filters_destroy(f);
	if (*act != 1) {
		free(val);
		return NULL;
	}
	return val;
}

/* what a query token takes: every stage */
char *
nxs_test_filter(const char *basedir, int stages, const char *s, int *act)
{
	return test_filter(basedir, stages, ~0u, s, act);
}

/* what a PREFIX takes: the normalizer only */
char *
nxs_test_filter_prefix(const char *basedir, int stages, const char *s, int *act)
{
	return test_filter(basedir, stages, NXS_FSTAGE_NORMALIZER, s, act);
}

/* host BK-tree image over a word list (ids 1..n), for structure tests */
int
nxs_test_bk_image(const char *const *words, uint32_t n_words, nxs_bkimage_t *out)
{
	hterm_t *terms = calloc((size_t)n_words + 2, sizeof(hterm_t));
	/* fake "nxsterms" bytes: every term points at a non-zero u64 total */
	static const uint8_t one[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1 };
	int r;

	for (uint32_t i = 0; i < n_words; i++) {
		bool dup = false;
		for (uint32_t j = 0; j < i && !dup; j++) {
			dup = strcmp(words[i], words[j]) == 0;
		}
		terms[i + 1].val = (const uint8_t *)words[i];
		terms[i + 1].len = (uint16_t)strlen(words[i]);
		terms[i + 1].tot_off = dup ? 0 : 8;
	}
	r = nxs_bk_build(terms, n_words, one, out);
	free(terms);
	return r;
}

int
nxs_test_levdist(const uint8_t *a, size_t n, const uint8_t *b, size_t m)
{
	extern int nxs_levdist_export(const uint8_t *, size_t, const uint8_t *, size_t);
	return nxs_levdist_export(a, n, b, m);
}

/*
 * The searches of nxs_explain.h on a list handed in (dt[0 .. n): doc << 32 | tf, ascending docs below n_docs):
 * for every docs[i], pos[i] = nxs_ex_find's answer (UINT64_MAX: absent) and lower[i] = nxs_ex_lower over the
 * whole list.  bitmap: through a block-presence bitmap and rank directory built here as the device index
 * builds its rows (k_blkmap_fill).  0 / -1 (out of memory).
 */
int
nxs_test_explain_search(const uint64_t *dt, uint64_t n, bool bitmap, uint32_t n_docs, const uint32_t *docs, size_t nd,
    uint64_t *pos, uint64_t *lower)
{
	const uint64_t words = ((uint64_t)n_docs + 4095) / 4096;
	uint64_t *bm = NULL;
	uint32_t *rk = NULL;

	if (bitmap) {
		bm = calloc(words ? words : 1, sizeof(uint64_t));
		rk = calloc(words + 1, sizeof(uint32_t));
		if (!bm || !rk) {
			free(bm);
			free(rk);
			return -1;
		}
		for (uint64_t w = 0, i = 0; w <= words; w++) {
			while (i < n && ((dt[i] >> 32) >> 12) < w) {
				i++;
			}
			rk[w] = (uint32_t)i;
		}
		for (uint64_t i = 0; i < n; i++) {
			const uint32_t d = (uint32_t)(dt[i] >> 32);
			bm[d >> 12] |= UINT64_C(1) << ((d >> 6) & 63);
		}
	}
	for (size_t i = 0; i < nd; i++) {
		pos[i] = docs[i] < n_docs ? nxs_ex_find(dt, 0, n, bm, rk, docs[i]) : nxs_ex_find(dt, 0, n, NULL, NULL, docs[i]);
		lower[i] = nxs_ex_lower(dt, 0, n, docs[i]);
	}
	free(bm);
	free(rk);
	return 0;
}

/*
 * nxs_dv_term (nxs_docterms.h) over the list dt[0 .. n) and the chunk ords[0 .. nd) (ascending, distinct, below
 * n_docs, nd <= NXS_DV_CHUNK); by_posting: 1 / 0 force the side, -1 = nxs_dv_by_posting's rule.  -> the side
 * taken (1: by posting), -1: out of memory / a chunk that is too long
 */
int
nxs_test_docterms_lane(const uint64_t *dt, uint64_t n, bool bitmap, uint32_t n_docs, const uint32_t *ords, uint32_t nd,
    int by_posting, uint64_t *pos)
{
	const uint64_t words = ((uint64_t)n_docs + 4095) / 4096;
	uint64_t *bm = NULL;
	uint32_t *rk = NULL;
	bool side;

	if (nd > NXS_DV_CHUNK) {
		return -1;
	}
	if (bitmap) {
		bm = calloc(words ? words : 1, sizeof(uint64_t));
		rk = calloc(words + 1, sizeof(uint32_t));
		if (!bm || !rk) {
			free(bm);
			free(rk);
			return -1;
		}
		for (uint64_t w = 0, i = 0; w <= words; w++) {
			while (i < n && ((dt[i] >> 32) >> 12) < w) {
				i++;
			}
			rk[w] = (uint32_t)i;
		}
		for (uint64_t i = 0; i < n; i++) {
			const uint32_t d = (uint32_t)(dt[i] >> 32);
			bm[d >> 12] |= UINT64_C(1) << ((d >> 6) & 63);
		}
	}
	side = by_posting < 0 ? nxs_dv_by_posting(n, nd, bitmap) : by_posting != 0;
	nxs_dv_term(dt, 0, n, bm, rk, ords, nd, side, pos);
	free(bm);
	free(rk);
	return side;
}

uint64_t
nxs_test_docterms_key(float w, uint32_t term)
{
	return nxs_dv_key(w, term);
}

/* nxs_related.h: the key of (c, df, term) under an order, the share, the predicate and the host ranker */
uint64_t
nxs_test_related_key(int order, uint32_t c, uint32_t df, uint32_t term)
{
	return nxs_rt_key(order, c, df, term);
}

float
nxs_test_related_share(uint32_t c, uint32_t df)
{
	return nxs_rt_share(c, df);
}

bool
nxs_test_related_eligible(uint32_t c, uint32_t df, uint32_t mincount, uint32_t mindf, uint32_t term, const uint32_t *excl,
    uint32_t n_excl)
{
	return nxs_rt_eligible(c, df, mincount, mindf, term, excl, n_excl);
}

int
nxs_test_related_rank(int order, const uint32_t *c, const uint32_t *df, uint32_t n_terms, uint32_t mincount,
    uint32_t mindf, const uint32_t *excl, uint32_t n_excl, uint32_t k, uint32_t *out_ids, uint64_t *matches)
{
	return nxs_rt_rank(order, c, df, n_terms, mincount, mindf, excl, n_excl, k, out_ids, matches);
}

/* nxs_matchdocs.h over caller arrays */
uint64_t
nxs_test_md_lower_bound(const uint64_t *ids, uint64_t n, uint64_t from)
{
	return nxs_md_lower_bound(ids, n, from);
}

uint64_t
nxs_test_md_page(const uint32_t *in_bits, const uint64_t *doc_ids, uint64_t D, uint64_t from, uint64_t limit,
    uint64_t *out, bool *more)
{
	return nxs_md_page(in_bits, doc_ids, D, from, limit, out, more);
}

/* nxs_docset.h: the set as the device wants it, and one lane of k_ds_score over arrays handed in */
size_t
nxs_test_docset_sort(uint64_t *ids, size_t n)
{
	return nxs_ds_sort_unique(ids, n);
}

/*
 * nxs_ds_lane over arrays handed in: nt lists back to back in dt / imp (list j = positions off[j] .. off[j + 1],
 * dt entries doc << 32 | tf, ascending by doc, docs below n_docs), the plan's truth table and program, and nd doc
 * ordinals.  bitmap: every list through a block-presence bitmap and rank directory built here as the device
 * index builds its rows.  hit[i] / score[i]: the lane's answer for ords[i].  0 / -1 (out of memory, nt > 32).
 */
int
nxs_test_docset_lane(const uint64_t *dt, const float *imp, const uint64_t *off, uint32_t nt, bool bitmap, uint32_t n_docs,
    const uint32_t *truth, const uint8_t *prog, uint32_t prog_len, const uint32_t *ords, size_t nd, uint8_t *hit,
    float *score)
{
	const uint64_t words = ((uint64_t)n_docs + 4095) / 4096, P = (nt && nt <= NXSGPU_MAX_TOKENS) ? off[nt] : 0;
	nxs_ds_tok_t toks[NXSGPU_MAX_TOKENS];
	nxs_ds_post_t *post = NULL;
	uint64_t *bm = NULL;
	uint32_t *rk = NULL;
	int ret = -1;

	if (nt > NXSGPU_MAX_TOKENS) {
		return -1;
	}
	post = calloc(P ? P : 1, sizeof(*post));
	bm = calloc((size_t)nt * (words ? words : 1) + 1, sizeof(uint64_t));
	rk = calloc((size_t)nt * (words + 1) + 1, sizeof(uint32_t));
	if (!post || !bm || !rk) {
		goto out;
	}
	for (uint64_t p = 0; p < P; p++) {
		post[p].doc = (uint32_t)(dt[p] >> 32);
		post[p].imp = imp[p];
	}
	for (uint32_t j = 0; j < nt; j++) {
		toks[j].beg = off[j];
		toks[j].end = off[j + 1];
		toks[j].row = bitmap ? j : NXS_DS_NONE;
		toks[j].pad = 0;
		for (uint64_t w = 0, i = off[j]; bitmap && w <= words; w++) {
			while (i < off[j + 1] && ((dt[i] >> 32) >> 12) < w) {
				i++;
			}
			rk[(size_t)j * (words + 1) + w] = (uint32_t)(i - off[j]);
		}
		for (uint64_t i = off[j]; bitmap && i < off[j + 1]; i++) {
			const uint32_t d = (uint32_t)(dt[i] >> 32);

			bm[(size_t)j * words + (d >> 12)] |= UINT64_C(1) << ((d >> 6) & 63);
		}
	}
	for (size_t i = 0; i < nd; i++) {
		score[i] = 0.0f;
		hit[i] = ords[i] < n_docs && nxs_ds_lane(ords[i], nt, toks, truth, prog, prog_len, dt, post, bm, rk, words, &score[i]);
	}
	ret = 0;
out:
	free(post);
	free(bm);
	free(rk);
	return ret;
}

/*
 * One part of the device index image (nxs_hooks.h): the host half only finds the device index and carries the
 * error over; the part is read where its arrays live (nxs_gpu_index.hip).  0, or -1 with the error declared.
 */
int
nxs_test_index_image(nxs_index_t *idx, int part, int algo, void *out, size_t cap, size_t *need)
{
	struct nxsgpu_index *dev = nxs_index_device(idx);

	*need = 0;
	if (!dev) {
		nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "the index has no device image");
		return -1;
	}
	if (nxsgpu_test_index_image(dev, part, algo, out, cap, need) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "%s", nxsgpu_last_error());
		return -1;
	}
	return 0;
}

/* ... and of the term-side state (nxs_hooks.h): read in nxs_gpu_fuzzy.hip and nxs_gpu_prefix.hip */
int
nxs_test_term_image(nxs_index_t *idx, int part, void *out, size_t cap, size_t *need)
{
	struct nxsgpu_index *dev = nxs_index_device(idx);

	*need = 0;
	if (!dev) {
		nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "the index has no device image");
		return -1;
	}
	if (nxsgpu_test_term_image(dev, part, out, cap, need) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "%s", nxsgpu_last_error());
		return -1;
	}
	return 0;
}

/* nxs_ex_ordinal for every q[i] over ids[0 .. n) (UINT64_MAX: not a live doc) */
void
nxs_test_explain_ordinal(const uint64_t *ids, uint64_t n, const uint64_t *q, size_t nq, uint64_t *out)
{
	for (size_t i = 0; i < nq; i++) {
		out[i] = nxs_ex_ordinal(ids, n, q[i]);
	}
}

/* the host ranker of completions (nxs_complete.h) over a dictionary handed in: term i has id i + 1 */
void
nxs_test_complete_host(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs, uint32_t n_terms,
    const uint8_t *prefix, size_t len, uint32_t k, uint32_t *out_ids, uint32_t *out_df, uint32_t *count,
    uint32_t *matches)
{
	nxs_complete_rank(terms, lens, dfs, NULL, n_terms, prefix, len, k, out_ids, out_df, count, matches);
}

/*
 * A query with prefix leaves against a dictionary handed in (words[i]: term id i + 1, df dfs[i]): prepare
 * (prefixmatch as given), resolve every prefix with the host ranker, splice.  -> the IR dump of the result
 * (nxs_query_repr; NULL on error), *n_prefix = the leaves read as prefixes, `prefixes` = their normalised
 * bytes in source order, one per line.
 */
char *
nxs_test_prefix_query(const char *query, const char *const *words, const uint32_t *dfs, uint32_t n_words,
    bool lowercase, bool prefixmatch, uint32_t prefix_limit, uint32_t *n_prefix, char *prefixes, size_t cap)
{
	nxs_index_t fake = { .lowercase = lowercase };
	const uint8_t **terms = calloc(n_words + 1, sizeof(*terms));
	uint32_t *lens = calloc(n_words + 1, sizeof(*lens));
	char *repr = NULL;
	size_t o = 0;
	qprep_t q;

	nxs_query_prepare_px(&fake, query, prefixmatch, &q);
	*n_prefix = (uint32_t)q.n_pfx;
	if (prefixes && cap) {
		prefixes[0] = '\0';
	}
	for (uint32_t w = 0; terms && lens && w < n_words; w++) {
		terms[w] = (const uint8_t *)words[w];
		lens[w] = (uint32_t)strlen(words[w]);
	}
	if (!q.errcode && terms && lens) {
		for (size_t i = q.n_pfx; i-- > 0; ) {
			qpfx_t *px = &q.pfx[i];
			uint32_t df[NXS_PREFIX_MAX], cnt = 0, m = 0;

			if (prefixes && o + px->len + 2 <= cap) {
				memcpy(prefixes + o, px->val, px->len);
				o += px->len;
				prefixes[o++] = '\n';
				prefixes[o] = '\0';
			}
			nxs_complete_rank(terms, lens, dfs, NULL, n_words, (const uint8_t *)px->val, px->len,
			    prefix_limit, px->ids, df, &cnt, &m);
			px->n = cnt;
			for (uint32_t e = 0; e < cnt; e++) {
				px->tval[e] = terms[px->ids[e] - 1];
				px->tlen[e] = (uint16_t)lens[px->ids[e] - 1];
			}
		}
		if (nxs_query_splice(&q) == 0) {
			repr = nxs_query_repr(&q.parse);
		}
	}
	nxs_query_release(&q);
	free(terms);
	free(lens);
	return repr;
}

/* the wildcard matcher alone (nxs_wild.h) */
int
nxs_test_wild_match(const uint8_t *term, size_t tlen, const uint8_t *pat, size_t plen)
{
	return nxs_wild_match(term, tlen, pat, plen);
}

/* ... as the device runs it: the first 8 bytes from a node's inline copy (zero padded), the rest from the pool */
int
nxs_test_wild_match_inl(const uint8_t *term, size_t tlen, const uint8_t *pat, size_t plen)
{
	uint8_t inl8[NXS_WILD_INL] = { 0 };
	uint64_t inl;

	memcpy(inl8, term, tlen < NXS_WILD_INL ? tlen : NXS_WILD_INL);
	memcpy(&inl, inl8, 8);
	return nxs_wild_match_inl(inl, NXS_WILD_INL, term, (uint32_t)tlen, pat, (uint32_t)plen);
}

/*
 * A pattern of `len` bytes (a NUL is a byte like any other) as nxs_index_wildcard normalises it
 * (nxs_wild_normalize) -> its result; on 1 the normalised bytes in out (at most cap), *out_len, *literals.
 */
int
nxs_test_wild_normalize(bool lowercase, const char *pat, size_t len, char *out, size_t cap, size_t *out_len,
    size_t *literals)
{
	nxs_index_t fake = { .lowercase = lowercase };
	char *val = NULL;
	const int r = nxs_wild_normalize(&fake, pat, len, &val, out_len, literals);

	if (r == 1) {
		memcpy(out, val, *out_len < cap ? *out_len : cap);
		free(val);
	}
	return r;
}

/* the host ranker of wildcard matches (nxs_wild.h) over a dictionary handed in: term i has id i + 1 */
void
nxs_test_wild_host(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs, uint32_t n_terms,
    const uint8_t *pat, size_t len, uint32_t k, uint32_t *out_ids, uint32_t *out_df, uint32_t *count,
    uint32_t *matches)
{
	nxs_wild_rank(terms, lens, dfs, NULL, n_terms, pat, len, k, out_ids, out_df, count, matches);
}

/*
 * A query with prefix and wildcard leaves against a dictionary handed in (words[i]: term id i + 1, df
 * dfs[i]): prepare (both flags as given), resolve every leaf with its host ranker, splice.  -> the IR dump
 * of the result (nxs_query_repr; NULL on error, *errcode = the query's), *n_leaves = the leaves read as
 * prefixes or patterns, `leaves` = one line per leaf in source order: `p` (prefix) or `w` (wildcard), a
 * blank and the normalised bytes.
 */
char *
nxs_test_wild_query(const char *query, const char *const *words, const uint32_t *dfs, uint32_t n_words,
    bool lowercase, bool prefixmatch, bool wildcardmatch, uint32_t prefix_limit, uint32_t wildcard_terms,
    uint32_t *n_leaves, char *leaves, size_t cap, int *errcode)
{
	nxs_index_t fake = { .lowercase = lowercase };
	const uint8_t **terms = calloc(n_words + 1, sizeof(*terms));
	uint32_t *lens = calloc(n_words + 1, sizeof(*lens));
	char *repr = NULL;
	size_t o = 0;
	qprep_t q;

	nxs_query_prepare_wc(&fake, query, prefixmatch, wildcardmatch, &q);
	*n_leaves = (uint32_t)q.n_pfx;
	*errcode = (int)q.errcode;
	if (leaves && cap) {
		leaves[0] = '\0';
	}
	for (uint32_t w = 0; terms && lens && w < n_words; w++) {
		terms[w] = (const uint8_t *)words[w];
		lens[w] = (uint32_t)strlen(words[w]);
	}
	if (!q.errcode && terms && lens) {
		for (size_t i = q.n_pfx; i-- > 0; ) {
			qpfx_t *px = &q.pfx[i];
			uint32_t df[NXS_PREFIX_MAX], cnt = 0, m = 0;

			if (leaves && o + px->len + 4 <= cap) {
				leaves[o++] = px->kind == QPFX_WILD ? 'w' : 'p';
				leaves[o++] = ' ';
				memcpy(leaves + o, px->val, px->len);
				o += px->len;
				leaves[o++] = '\n';
				leaves[o] = '\0';
			}
			if (px->kind == QPFX_WILD) {
				nxs_wild_rank(terms, lens, dfs, NULL, n_words, (const uint8_t *)px->val, px->len,
				    wildcard_terms, px->ids, df, &cnt, &m);
			} else {
				nxs_complete_rank(terms, lens, dfs, NULL, n_words, (const uint8_t *)px->val, px->len,
				    prefix_limit, px->ids, df, &cnt, &m);
			}
			px->n = cnt;
			for (uint32_t e = 0; e < cnt; e++) {
				px->tval[e] = terms[px->ids[e] - 1];
				px->tlen[e] = (uint16_t)lens[px->ids[e] - 1];
			}
		}
		if (nxs_query_splice(&q) == 0) {
			repr = nxs_query_repr(&q.parse);
		}
	}
	nxs_query_release(&q);
	free(terms);
	free(lens);
	return repr;
}

/* the host ranker (nxs_suggest.h) over a dictionary handed in: term i has id i + 1 */
void
nxs_test_suggest_host(const uint8_t *const *terms, const uint32_t *lens, const uint32_t *dfs, uint32_t n_terms,
    const uint8_t *token, size_t len, uint32_t maxdist, uint32_t k, uint32_t *out_ids, uint8_t *out_dist,
    uint32_t *out_df, uint32_t *count, uint32_t *matches)
{
	nxs_suggest_rank(terms, lens, dfs, NULL, n_terms, token, len, maxdist, k, out_ids, out_dist, out_df, count, matches);
}
#endif /* NXS_TEST_HOOKS */
