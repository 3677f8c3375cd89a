/*
 * nxs_resp.c -- the response object (nxs_resp_*): the slab a batch's responses
 * live in, the accessors, the JSON writer, and the explanations attached to them.
 *   response object       src/core/results.c:46-246
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"
#include "nxs_explain.h"

/*
 * The responses of one batch live in ONE allocation (the reference's
 * nxs_resp_create mallocs a map, a heap and a JSON document per query,
 * results.c:46-85): header + n response structs + all (id, score) pairs.  Each
 * nxs_resp_t stays individually releasable; the slab goes with the last one.
 */
int
slab_begin(slab_builder_t *b, size_t n, size_t total)
{
	const size_t hdr = (sizeof(struct resp_slab) + 15) & ~(size_t)15;
	const size_t rs = (n * sizeof(nxs_resp_t) + 15) & ~(size_t)15;
	uint8_t *m = malloc(hdr + rs + total * sizeof(nxs_doc_id_t) + total * sizeof(float) + 16);

	if (!m) {
		return -1;
	}
	b->slab = (struct resp_slab *)m;
	b->slab->refs = 0;
	b->slab->ex = NULL;
	b->resps = (nxs_resp_t *)(m + hdr);
	b->ids = (nxs_doc_id_t *)(m + hdr + rs);
	b->scores = (float *)(b->ids + total);
	b->used = 0;
	return 0;
}

void
slab_free(struct resp_slab *s)
{
	free(s->ex);
	free(s);
}

void
nxs_resp_release(nxs_resp_t *r)
{
	if (r->slab) {
		if (--r->slab->refs == 0) {
			slab_free(r->slab);
		}
		return;
	}
	free(r->ids);
	free(r->scores);
	free(r);
}

void
nxs_resp_iter_reset(nxs_resp_t *r)
{
	r->iter = 0;
}

bool
nxs_resp_iter_result(nxs_resp_t *r, nxs_doc_id_t *doc_id, float *score)
{
	if (r->iter >= r->count) {
		return false;
	}
	*doc_id = r->ids[r->iter];
	*score = r->scores[r->iter];	/* float -> JSON double -> float is exact */
	r->iter++;
	return true;
}

unsigned
nxs_resp_resultcount(const nxs_resp_t *r)
{
	return r->count;
}

bool
nxs_resp_total(const nxs_resp_t *r, uint64_t *total)
{
	if (!r->has_total) {
		return false;
	}
	*total = r->total;
	return true;
}

/*
 * JSON real: shortest decimal that round-trips (double)score, always with a
 * fraction digit -- what yyjson's writer produces for results.c:158.  Pinned
 * by the reference only for 3.0 and 1.5 (t_misc.c:115-117).
 */
size_t
fmt_real(char *out, double v)
{
	char e[40], digs[24];
	int nd = 0, x, prec;
	size_t o = 0;
	const char *p, *ep;

	for (prec = 1; prec <= 17; prec++) {
		snprintf(e, sizeof(e), "%.*e", prec - 1, v);
		if (strtod(e, NULL) == v) {
			break;
		}
	}
	p = e;
	if (*p == '-') {
		out[o++] = '-';
		p++;
	}
	ep = strchr(p, 'e');
	for (; p < ep; p++) {
		if (*p != '.') {
			digs[nd++] = *p;
		}
	}
	while (nd > 1 && digs[nd - 1] == '0') {
		nd--;
	}
	x = atoi(ep + 1);
	if (x >= -6 && x < 21) {
		if (x < 0) {
			out[o++] = '0';
			out[o++] = '.';
			for (int i = 0; i < -x - 1; i++) out[o++] = '0';
			for (int i = 0; i < nd; i++) out[o++] = digs[i];
		} else {
			for (int i = 0; i <= x; i++) out[o++] = i < nd ? digs[i] : '0';
			out[o++] = '.';
			if (nd > x + 1) {
				for (int i = x + 1; i < nd; i++) out[o++] = digs[i];
			} else {
				out[o++] = '0';
			}
		}
	} else {
		out[o++] = digs[0];
		if (nd > 1) {
			out[o++] = '.';
			for (int i = 1; i < nd; i++) out[o++] = digs[i];
		}
		o += sprintf(out + o, "e%d", x);
	}
	out[o] = '\0';
	return o;
}

unsigned
nxs_resp_tokens(const nxs_resp_t *r)
{
	return r->n_tok;
}

bool
nxs_resp_token(const nxs_resp_t *r, unsigned j, const char **term, size_t *len)
{
	if (j >= r->n_tok) {
		return false;
	}
	if (term) {
		*term = r->tok[j];
	}
	if (len) {
		*len = r->tok_len[j];
	}
	return true;
}

bool
nxs_resp_explain(const nxs_resp_t *r, unsigned i, unsigned j, float *score, uint32_t *tf)
{
	size_t at;

	if (i >= r->count || j >= r->n_tok) {
		return false;
	}
	at = (size_t)i * r->n_tok + j;
	if (r->ex_tf[at] == 0) {
		return false;
	}
	if (score) {
		*score = r->ex_imp[at];
	}
	if (tf) {
		*tf = r->ex_tf[at];
	}
	return true;
}

/*
 * {"results":[{"doc_id":N,"score":X},...],"count":K}  (results.c:80-82,153-161,218); with "total" it ends
 * ...,"total":M}; an explained response (new) carries per result "terms":[{"t":J,"tf":N,"score":X},...] -- the
 * present tokens in ascending J -- and ends ...,"tokens":["term",...]}
 */
char *
nxs_resp_tojson(nxs_resp_t *r, size_t *len)
{
	size_t cap = 80 + (size_t)r->count * 88;
	char *s;
	size_t o = 0;

	if (r->explained) {
		cap += 16 + (size_t)r->count * (16 + (size_t)r->n_tok * 72);
		for (unsigned j = 0; j < r->n_tok; j++) {
			cap += 4 + 6 * (size_t)r->tok_len[j];
		}
	}
	if ((s = malloc(cap)) == NULL) {
		return NULL;
	}
	o += sprintf(s + o, "{\"results\":[");
	for (unsigned i = 0; i < r->count; i++) {
		o += sprintf(s + o, "%s{\"doc_id\":%llu,\"score\":", i ? "," : "",
		    (unsigned long long)r->ids[i]);
		o += fmt_real(s + o, (double)r->scores[i]);
		if (r->explained) {
			const char *sep = "";

			o += sprintf(s + o, ",\"terms\":[");
			for (unsigned j = 0; j < r->n_tok; j++) {
				const size_t at = (size_t)i * r->n_tok + j;

				if (r->ex_tf[at] == 0) {
					continue;
				}
				o += sprintf(s + o, "%s{\"t\":%u,\"tf\":%u,\"score\":", sep, j, r->ex_tf[at]);
				o += fmt_real(s + o, (double)r->ex_imp[at]);
				s[o++] = '}';
				sep = ",";
			}
			s[o++] = ']';
		}
		s[o++] = '}';
	}
	if (r->has_total) {
		o += sprintf(s + o, "],\"count\":%u,\"total\":%llu", r->count, (unsigned long long)r->total);
	} else {
		o += sprintf(s + o, "],\"count\":%u", r->count);
	}
	if (r->explained) {
		o += sprintf(s + o, ",\"tokens\":[");
		for (unsigned j = 0; j < r->n_tok; j++) {
			if (j) {
				s[o++] = ',';
			}
			o += json_str(s + o, r->tok[j], r->tok_len[j]);
		}
		s[o++] = ']';
	}
	s[o++] = '}';
	s[o] = '\0';
	if (len) {
		*len = o;
	}
	return s;
}

/* a JSON string: UTF-8 passes through; '"', '\\' and bytes < 0x20 (as \u00XX) are escaped */
size_t
json_str(char *out, const char *s, size_t n)
{
	size_t o = 0;

	out[o++] = '"';
	for (size_t i = 0; i < n; i++) {
		const unsigned char c = (unsigned char)s[i];
		if (c == '"' || c == '\\') {
			out[o++] = '\\';
			out[o++] = (char)c;
		} else if (c < 0x20) {
			o += (size_t)sprintf(out + o, "\\u%04x", c);
		} else {
			out[o++] = (char)c;
		}
	}
	out[o++] = '"';
	return o;
}

/* ---- explanations ("explain") --------------------------------------------------------- */

/*
 * Explanations of a batch's responses: ONE nxsgpu_explain call per device index for all of them, on the
 * final results (after exact re-queries) and before the device index can move.  `shards`: the index, or the
 * doc shards of a collection -- they hold disjoint docs, so every result's row comes from the one shard
 * whose `found` is set (none, or two: NXS_ERR_FATAL).  The dictionary is shards[0]'s (the same on every
 * shard); term bytes are copied by term id, so a plan from the plan cache explains like a parsed one.
 * Everything lands in one block that the responses' slab owns.  Responses with no result keep n_tok == 0.
 * 0, or -1 with the error declared (the responses are untouched then).
 */
int
explain_attach(nxs_index_t *const *shards, unsigned n_shards, int algo, const ex_item_t *items, size_t n_items,
    struct resp_slab *slab)
{
	const nxs_index_t *dict = shards[0];
	nxs_t *nxs = dict->nxs;
	uint32_t *tok_off = NULL, *tok_ids = NULL, *s_tf = NULL;
	uint64_t *res_off = NULL, *doc_ids = NULL;
	float *s_imp = NULL;
	uint8_t *found = NULL, *seen = NULL, *blk = NULL;
	size_t n_tok = 0, n_res = 0, cells = 0, bytes = 0, nq = 0, o;
	int ret = -1;

	for (size_t i = 0; i < n_items; i++) {
		const ex_item_t *it = &items[i];

		if (!it->r->count || !it->n_tok) {
			continue;
		}
		for (uint32_t j = 0; j < it->n_tok; j++) {
			if (it->term_ids[j] < 1 || it->term_ids[j] > dict->last_id) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "explain: a plan names term %u, which the dictionary lacks",
				    it->term_ids[j]);
				return -1;
			}
			bytes += (size_t)dict->terms[it->term_ids[j]].len + 1;
		}
		nq++;
		n_tok += it->n_tok;
		n_res += it->r->count;
		cells += (size_t)it->r->count * it->n_tok;
	}
	if (nq == 0) {
		return 0;
	}
	if (nq > UINT32_MAX - 1 || n_tok > UINT32_MAX / 2) {
		nxs_decl_err(nxs, NXS_ERR_LIMIT, "explain: batch too large");
		return -1;
	}
	tok_off = malloc((nq + 1) * sizeof(uint32_t));
	tok_ids = malloc(n_tok * sizeof(uint32_t));
	res_off = malloc((nq + 1) * sizeof(uint64_t));
	doc_ids = malloc(n_res * sizeof(uint64_t));
	found = malloc(n_res);
	/* block: term pointers | tf | contributions | term lengths | term bytes */
	const size_t o_tf = n_tok * sizeof(char *), o_imp = o_tf + cells * 4, o_len = o_imp + cells * 4,
	    o_bytes = o_len + n_tok * 4;
	blk = malloc(o_bytes + bytes + 1);
	if (n_shards > 1) {
		s_tf = malloc(cells * sizeof(uint32_t));
		s_imp = malloc(cells * sizeof(float));
		seen = calloc(n_res, 1);
	}
	if (!tok_off || !tok_ids || !res_off || !doc_ids || !found || !blk ||
	    (n_shards > 1 && (!s_tf || !s_imp || !seen))) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	const char **b_tok = (const char **)blk;
	uint32_t *b_tf = (uint32_t *)(blk + o_tf), *b_len = (uint32_t *)(blk + o_len);
	float *b_imp = (float *)(blk + o_imp);
	char *b_bytes = (char *)(blk + o_bytes);

	tok_off[0] = 0;
	res_off[0] = 0;
	o = 0;
	for (size_t i = 0, q = 0; i < n_items; i++) {
		const ex_item_t *it = &items[i];

		if (!it->r->count || !it->n_tok) {
			continue;
		}
		for (uint32_t j = 0; j < it->n_tok; j++) {
			const hterm_t *t = &dict->terms[it->term_ids[j]];
			const size_t at = tok_off[q] + j;

			tok_ids[at] = it->term_ids[j];
			b_tok[at] = b_bytes + o;
			b_len[at] = t->len;
			memcpy(b_bytes + o, t->val, t->len);
			b_bytes[o + t->len] = '\0';
			o += (size_t)t->len + 1;
		}
		memcpy(doc_ids + res_off[q], it->r->ids, (size_t)it->r->count * sizeof(uint64_t));
		tok_off[q + 1] = tok_off[q] + it->n_tok;
		res_off[q + 1] = res_off[q] + it->r->count;
		q++;
	}
	if (n_shards == 1) {
		if (nxsgpu_explain(shards[0]->dev, algo, (uint32_t)nq, tok_off, tok_ids, res_off, doc_ids, b_tf, b_imp, found) != 0) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "device explain failed: %s", nxsgpu_last_error());
			goto out;
		}
		for (size_t r = 0; r < n_res; r++) {
			if (!found[r]) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "explain: doc %llu was returned but is not in the index",
				    (unsigned long long)doc_ids[r]);
				goto out;
			}
		}
	} else {
		for (unsigned s = 0; s < n_shards; s++) {
			if (nxsgpu_explain(shards[s]->dev, algo, (uint32_t)nq, tok_off, tok_ids, res_off, doc_ids, s_tf, s_imp, found) != 0) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "device explain failed on shard %u: %s", s, nxsgpu_last_error());
				goto out;
			}
			for (size_t q = 0, c = 0; q < nq; q++) {
				const size_t nt = tok_off[q + 1] - tok_off[q];

				for (uint64_t r = res_off[q]; r < res_off[q + 1]; r++, c += nt) {
					if (!found[r]) {
						continue;
					}
					if (seen[r]) {
						nxs_decl_err(nxs, NXS_ERR_FATAL, "explain: doc %llu is held by two shards",
						    (unsigned long long)doc_ids[r]);
						goto out;
					}
					seen[r] = 1;
					memcpy(b_tf + c, s_tf + c, nt * 4);
					memcpy(b_imp + c, s_imp + c, nt * 4);
				}
			}
		}
		for (size_t r = 0; r < n_res; r++) {
			if (!seen[r]) {
				nxs_decl_err(nxs, NXS_ERR_FATAL, "explain: doc %llu was returned but no shard holds it",
				    (unsigned long long)doc_ids[r]);
				goto out;
			}
		}
	}
	for (size_t i = 0, q = 0, c = 0; i < n_items; i++) {
		const ex_item_t *it = &items[i];
		nxs_resp_t *r = it->r;

		if (!r->count || !it->n_tok) {
			continue;
		}
		r->n_tok = it->n_tok;
		r->tok = b_tok + tok_off[q];
		r->tok_len = b_len + tok_off[q];
		r->ex_tf = b_tf + c;
		r->ex_imp = b_imp + c;
		c += (size_t)r->count * it->n_tok;
		q++;
	}
	slab->ex = blk;
	blk = NULL;
	ret = 0;
out:
	free(tok_off); free(tok_ids); free(res_off); free(doc_ids); free(found);
	free(s_tf); free(s_imp); free(seen); free(blk);
	return ret;
}

#ifdef NXS_TEST_HOOKS
/*
 * A response built by hand (accessors and JSON without an index): `count` results; explained: n_tok tokens
 * (terms / lens) and the cells tf / imp [count][n_tok], tf == 0 = absent.  NULL: out of memory.
 */
nxs_resp_t *
nxs_test_resp_build(unsigned count, const uint64_t *ids, const float *scores, bool has_total, uint64_t total,
    bool explained, unsigned n_tok, const uint8_t *const *terms, const size_t *lens, const uint32_t *tf,
    const float *imp)
{
	slab_builder_t sb = { 0 };
	nxs_resp_t *r;
	size_t bytes = 0, o = 0;
	const size_t cells = (size_t)count * n_tok;

	if (slab_begin(&sb, 1, count) == -1) {
		return NULL;
	}
	r = slab_resp(&sb, 0, count);
	memcpy(r->ids, ids, (size_t)count * sizeof(uint64_t));
	memcpy(r->scores, scores, (size_t)count * sizeof(float));
	r->has_total = has_total;
	r->total = total;
	r->explained = explained;
	if (explained && n_tok) {
		for (unsigned j = 0; j < n_tok; j++) {
			bytes += lens[j] + 1;
		}
		const size_t o_tf = n_tok * sizeof(char *), o_imp = o_tf + cells * 4, o_len = o_imp + cells * 4,
		    o_bytes = o_len + (size_t)n_tok * 4;
		uint8_t *blk = malloc(o_bytes + bytes + 1);

		if (!blk) {
			nxs_resp_release(r);
			return NULL;
		}
		const char **b_tok = (const char **)blk;
		uint32_t *b_len = (uint32_t *)(blk + o_len);
		char *b_bytes = (char *)(blk + o_bytes);

		memcpy(blk + o_tf, tf, cells * 4);
		memcpy(blk + o_imp, imp, cells * 4);
		for (unsigned j = 0; j < n_tok; j++) {
			b_tok[j] = b_bytes + o;
			b_len[j] = (uint32_t)lens[j];
			memcpy(b_bytes + o, terms[j], lens[j]);
			b_bytes[o + lens[j]] = '\0';
			o += lens[j] + 1;
		}
		r->n_tok = n_tok;
		r->tok = b_tok;
		r->tok_len = b_len;
		r->ex_tf = (const uint32_t *)(blk + o_tf);
		r->ex_imp = (const float *)(blk + o_imp);
		sb.slab->ex = blk;
	}
	return r;
}
#endif /* NXS_TEST_HOOKS */
