/*
 * nxs_lookup.c -- dictionary lookups by string: spelling suggestions
 * (nxs_index_suggest), prefix completions (nxs_index_complete) and wildcard
 * matches (nxs_index_wildcard); by doc: its term vector (nxs_index_doc_terms);
 * by query: the terms of its matches (nxs_index_related); and the object all
 * five return (nxs_sugg_t).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"
#include "nxs_suggest.h"
#include "nxs_wild.h"

/* ---- the object of the calls (nxs_sugg_t)  --------------------------------------------- */

typedef struct {
	char *		term;		/* owned by the object, NUL-terminated */
	size_t		len;
	unsigned	dist;		/* (a term vector's: the doc's term count) */
	uint64_t	df;
	float		score;		/* a term vector's: rank(term, doc); a related term's: its share c / df */
} sugg_item_t;

struct nxs_sugg {
	char *		token;		/* the token after the filters (empty when dropped) */
	size_t		token_len;
	bool		dropped;
	int		kind;		/* SUGG_*: by nxs_index_complete / _wildcard `token` is the prefix / the pattern, the
					 * JSON has its own shape; by nxs_index_doc_terms there is no string but doc_id; by
					 * nxs_index_related `token` is the query as given, dist = c, docs = |M| */
	uint64_t	doc_id;
	uint64_t	docs;
	uint64_t	matches;
	unsigned	count;
	sugg_item_t	items[];
};

enum { SUGG_SUGGEST = 0, SUGG_COMPLETE = 1, SUGG_WILD = 2, SUGG_DOC = 3, SUGG_RELATED = 4 };

/* one block: the object, its items, the strings */
static nxs_sugg_t *
sugg_build(const char *token, size_t token_len, bool dropped, uint64_t matches, unsigned count,
    const uint8_t *const *terms, const size_t *lens, const unsigned *dists, const uint64_t *dfs)
{
	size_t bytes = sizeof(nxs_sugg_t) + count * sizeof(sugg_item_t) + token_len + 1;
	nxs_sugg_t *sg;
	char *str;

	for (unsigned i = 0; i < count; i++) {
		bytes += lens[i] + 1;
	}
	if ((sg = malloc(bytes)) == NULL) {
		return NULL;
	}
	str = (char *)&sg->items[count];
	sg->token = str;
	sg->token_len = token_len;
	memcpy(str, token, token_len);
	str[token_len] = '\0';
	str += token_len + 1;
	sg->dropped = dropped;
	sg->kind = SUGG_SUGGEST;
	sg->doc_id = 0;
	sg->docs = 0;
	sg->matches = matches;
	sg->count = count;
	for (unsigned i = 0; i < count; i++) {
		sg->items[i].term = str;
		sg->items[i].len = lens[i];
		sg->items[i].dist = dists[i];
		sg->items[i].df = dfs[i];
		sg->items[i].score = 0.0f;
		memcpy(str, terms[i], lens[i]);
		str[lens[i]] = '\0';
		str += lens[i] + 1;
	}
	return sg;
}

unsigned
nxs_sugg_count(const nxs_sugg_t *sg)
{
	return sg->count;
}

uint64_t
nxs_sugg_matches(const nxs_sugg_t *sg)
{
	return sg->matches;
}

bool
nxs_sugg_dropped(const nxs_sugg_t *sg)
{
	return sg->dropped;
}

bool
nxs_sugg_get(const nxs_sugg_t *sg, unsigned i, const char **term, size_t *len, unsigned *distance, uint64_t *df)
{
	if (i >= sg->count) {
		return false;
	}
	if (term) *term = sg->items[i].term;
	if (len) *len = sg->items[i].len;
	if (distance) *distance = sg->items[i].dist;
	if (df) *df = sg->items[i].df;
	return true;
}

bool
nxs_sugg_score(const nxs_sugg_t *sg, unsigned i, float *score)
{
	if ((sg->kind != SUGG_DOC && sg->kind != SUGG_RELATED) || i >= sg->count) {
		return false;
	}
	if (score) *score = sg->items[i].score;
	return true;
}

bool
nxs_sugg_docs(const nxs_sugg_t *sg, uint64_t *docs)
{
	if (sg->kind != SUGG_RELATED) {
		return false;
	}
	if (docs) *docs = sg->docs;
	return true;
}

void
nxs_sugg_release(nxs_sugg_t *sg)
{
	free(sg);
}

/* {"token":"...","suggestions":[{"term":"...","distance":D,"df":N},...],"matches":M}; of a completion:
 * {"prefix":"...","completions":[{"term":"...","df":N},...],"matches":M}; of a wildcard match:
 * {"pattern":"...","terms":[{"term":"...","df":N},...],"matches":M}; of a term vector:
 * {"doc_id":N,"terms":[{"term":"...","tf":N,"df":N,"score":X},...],"matches":M}; of related terms:
 * {"query":"...","docs":N,"terms":[{"term":"...","count":N,"df":N,"score":X},...],"matches":M} */
char *
nxs_sugg_tojson(nxs_sugg_t *sg, size_t *len)
{
	static const char *const head[] = { "{\"token\":", "{\"prefix\":", "{\"pattern\":", "", "{\"query\":" };
	static const char *const list[] = { ",\"suggestions\":[", ",\"completions\":[", ",\"terms\":[", ",\"terms\":[", ",\"terms\":[" };
	size_t cap = 128 + 6 * sg->token_len, o = 0;
	char *s;

	for (unsigned i = 0; i < sg->count; i++) {
		cap += 112 + 6 * sg->items[i].len;
	}
	if ((s = malloc(cap)) == NULL) {
		return NULL;
	}
	if (sg->kind == SUGG_DOC) {
		o += (size_t)sprintf(s + o, "{\"doc_id\":%llu", (unsigned long long)sg->doc_id);
	} else {
		o += (size_t)sprintf(s + o, "%s", head[sg->kind]);
		o += json_str(s + o, sg->token, sg->token_len);
		if (sg->kind == SUGG_RELATED) {
			o += (size_t)sprintf(s + o, ",\"docs\":%llu", (unsigned long long)sg->docs);
		}
	}
	o += (size_t)sprintf(s + o, "%s", list[sg->kind]);
	for (unsigned i = 0; i < sg->count; i++) {
		o += (size_t)sprintf(s + o, "%s{\"term\":", i ? "," : "");
		o += json_str(s + o, sg->items[i].term, sg->items[i].len);
		if (sg->kind == SUGG_DOC || sg->kind == SUGG_RELATED) {
			o += (size_t)sprintf(s + o, ",\"%s\":%u,\"df\":%llu,\"score\":", sg->kind == SUGG_DOC ? "tf" : "count",
			    sg->items[i].dist, (unsigned long long)sg->items[i].df);
			o += fmt_real(s + o, (double)sg->items[i].score);
			s[o++] = '}';
		} else if (sg->kind != SUGG_SUGGEST) {
			o += (size_t)sprintf(s + o, ",\"df\":%llu}", (unsigned long long)sg->items[i].df);
		} else {
			o += (size_t)sprintf(s + o, ",\"distance\":%u,\"df\":%llu}", sg->items[i].dist,
			    (unsigned long long)sg->items[i].df);
		}
	}
	o += (size_t)sprintf(s + o, "],\"matches\":%llu}", (unsigned long long)sg->matches);
	if (len) {
		*len = o;
	}
	return s;
}

/* ---- the path the calls take: enter, stage, pack, (the device call), build ------------------------- */

/* the strings of one call: what the filters made of them, the kept ones packed for the device, its answers */
typedef struct {
	size_t		n;
	struct lookup_str {
		char *	val;		/* after the filters (owned) */
		size_t	len;
		int	act;		/* 1 = goes to the device, 0 = does not (the caller says what that means),
					 * < 0 = the filters failed */
	} *		s;		/* [n] */
	size_t		nd;		/* strings packed: those with act == 1, in order */
	uint8_t *	bytes;		/* back to back ... */
	uint32_t *	off;		/* ... [nd + 1] */
	uint32_t	*ids, *df;	/* the device's answers: [nd * k], */
	uint8_t *	dist;		/* [nd * k] (suggest only), */
	uint32_t	*counts, *matches;	/* [nd] */
} lookup_t;

static void
lookup_free(lookup_t *st)
{
	for (size_t i = 0; st->s && i < st->n; i++) {
		free(st->s[i].val);
	}
	free(st->s);
	free(st->off);
	free(st->bytes);
	free(st->ids);
	free(st->df);
	free(st->dist);
	free(st->counts);
	free(st->matches);
}

/* what comes before the strings are looked at, and after the caller has read its params (bk: the call reads
 * the BK image).  0 / -1 */
int
lookup_enter(nxs_index_t *idx, const char *what, size_t n, bool bk)
{
	nxs_t *nxs = idx->nxs;

	/* (a shard's dictionary and df are collection-wide, its postings are not: a follow-up, include/nxs.h) */
	if (idx->n_shards) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "%s is not available on a doc shard", what);
		return -1;
	}
	if (n > UINT32_MAX / 2) {
		nxs_decl_err(nxs, NXS_ERR_LIMIT, "batch too large");
		return -1;
	}
	/*
	 * search.c:309-312, as every search does.  The call is local: with a communicator attached the
	 * batches in flight can only be finished by all ranks together (resync_before_batch), so while
	 * some are in flight this rank answers from the snapshot they run on.
	 */
	if (!(idx->comm && pend_oldest(idx)) && resync_before_batch(idx) == -1) {
		return -1;
	}
	/* new terms reach the BK image first.  (A batch whose fuzzy pass is still on the device reads the
	 * image: it was synced for that pass, and nothing can have moved since without finishing the batch --
	 * should the image be stale all the same, the pass is waited for before it is replaced.) */
	if (bk && (idx->bk_upto != idx->last_id || idx->bk_flags_stale)) {
		(void)late_finish(idx);
		if (nxs_index_bk_sync(idx) == -1) {
			return -1;
		}
	}
	return 0;
}

/* a copy of every string through the index's filters on `stages` (lens: NULL = NUL-terminated).  0 / -1 */
static int
lookup_stage(nxs_index_t *idx, const char *const *strings, const size_t *lens, size_t n, unsigned stages,
    lookup_t *st)
{
	st->n = n;
	if ((st->s = calloc(n ? n : 1, sizeof(*st->s))) == NULL) {
		goto oom;
	}
	for (size_t i = 0; i < n; i++) {
		struct lookup_str *e = &st->s[i];

		e->len = lens ? lens[i] : strlen(strings[i]);
		if ((e->val = malloc(e->len + 1)) == NULL) {
			goto oom;
		}
		memcpy(e->val, strings[i], e->len);
		e->val[e->len] = '\0';
		e->act = nxs_index_filter(idx, stages, &e->val, &e->len);
	}
	return 0;
oom:
	nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
	return -1;
}

/* the strings with act == 1 as the device reads them, and room for its k answers to each.  0 / -1 */
static int
lookup_pack(nxs_t *nxs, lookup_t *st, unsigned k)
{
	size_t blen = 0, nd = 0;

	for (size_t i = 0; i < st->n; i++) {
		if (st->s[i].act == 1) {
			blen += st->s[i].len;
			nd++;
		}
	}
	if (blen > UINT32_MAX / 2) {
		nxs_decl_err(nxs, NXS_ERR_LIMIT, "batch too large");
		return -1;
	}
	st->off = malloc((nd + 1) * sizeof(*st->off));
	st->bytes = malloc(blen + 16);
	st->ids = malloc((nd * k + 1) * sizeof(*st->ids));
	st->df = malloc((nd * k + 1) * sizeof(*st->df));
	st->dist = malloc(nd * k + 1);
	st->counts = malloc((nd + 1) * sizeof(*st->counts));
	st->matches = malloc((nd + 1) * sizeof(*st->matches));
	if (!st->off || !st->bytes || !st->ids || !st->df || !st->dist || !st->counts || !st->matches) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		return -1;
	}
	blen = 0;
	for (size_t i = 0; i < st->n; i++) {
		if (st->s[i].act == 1) {
			st->off[st->nd++] = (uint32_t)blen;
			memcpy(st->bytes + blen, st->s[i].val, st->s[i].len);
			blen += st->s[i].len;
		}
	}
	st->off[st->nd] = (uint32_t)blen;
	return 0;
}

/*
 * String i's object from the device's answer to packed string *nd (stepped here), or its failure: NULL with
 * errs[i] and the error set.  `noun` names the string in messages.  dist == NULL: the device sends no
 * distances -- every term holds the string's `lit` literal bytes (a prefix: all of it, and the pair's true
 * Levenshtein distance is what the term adds), and the distance reported is what it holds beyond them.
 */
static nxs_sugg_t *
lookup_build(nxs_index_t *idx, const lookup_t *st, size_t i, size_t *nd, unsigned k, const uint8_t *dist,
    size_t lit, const char *noun, nxs_err_t *errs)
{
	const uint8_t *terms[NXS_SUGGEST_MAX];
	size_t tlens[NXS_SUGGEST_MAX];
	unsigned dists[NXS_SUGGEST_MAX];
	uint64_t dfs[NXS_SUGGEST_MAX];
	nxs_err_t code = NXS_ERR_FATAL;
	nxs_sugg_t *sg;
	size_t at;
	unsigned c;

	if (st->s[i].act < 0) {
		/* FILT_ERROR: what fails a query (search.c:199-203) fails this string */
		nxs_decl_err(idx->nxs, code, "the filters failed on %s %zu", noun, i);
		goto fail;
	}
	at = (*nd)++;
	/* (count = min(k, matches) is the device's contract, k <= NXS_SUGGEST_MAX the params': the arrays hold it) */
	c = st->counts[at] <= k ? st->counts[at] : k;
	for (unsigned j = 0; j < c; j++) {
		const uint32_t id = st->ids[at * k + j];

		if (id < 1 || id > idx->last_id || (!dist && idx->terms[id].len < lit)) {
			nxs_decl_err(idx->nxs, code, "the device named an unknown term for %s %zu", noun, i);
			goto fail;
		}
		terms[j] = idx->terms[id].val;
		tlens[j] = idx->terms[id].len;
		dists[j] = dist ? dist[at * k + j] : (unsigned)(tlens[j] - lit);
		dfs[j] = st->df[at * k + j];
	}
	if ((sg = sugg_build(st->s[i].val, st->s[i].len, false, st->matches[at], c, terms, tlens, dists, dfs)) != NULL) {
		return sg;
	}
	code = NXS_ERR_SYSTEM;
	nxs_decl_err(idx->nxs, code, "out of memory");
fail:
	if (errs) {
		errs[i] = code;
	}
	return NULL;
}

/* ---- spelling suggestions (nxs_index_suggest) ---------------------------------------- */

/* `key`: how many terms a call returns (1..NXS_SUGGEST_MAX, default 5) */
static int
get_limit_param(nxs_t *nxs, const nxs_params_t *params, const char *key, unsigned *k)
{
	uint64_t v;

	*k = 5;
	if (params && nxs_params_get_uint(params, key, &v) == 0) {
		if (v < 1 || v > NXS_SUGGEST_MAX) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid %s (1..%d)", key, NXS_SUGGEST_MAX);
			return -1;
		}
		*k = (unsigned)v;
	}
	return 0;
}

/* "suggest_limit", "suggest_maxdist" (1 or 2, default 2) */
static int
get_suggest_params(nxs_t *nxs, const nxs_params_t *params, unsigned *k, unsigned *maxdist)
{
	uint64_t v;

	*maxdist = LEVDIST_TOLERANCE;
	if (get_limit_param(nxs, params, "suggest_limit", k) == -1) {
		return -1;
	}
	if (params && nxs_params_get_uint(params, "suggest_maxdist", &v) == 0) {
		if (v < 1 || v > LEVDIST_TOLERANCE) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid suggest_maxdist (1 or 2)");
			return -1;
		}
		*maxdist = (unsigned)v;
	}
	return 0;
}

/* lens: NULL = the strings are NUL-terminated */
static int
suggest_run(nxs_index_t *idx, nxs_params_t *params, const char *const *tokens, const size_t *lens, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	lookup_t st = { 0 };
	unsigned k, maxdist;
	size_t nd = 0;
	int ret = -1, failed = 0;

	nxs_clear_error(nxs);
	outs_clear(out, errs, n);
	if (get_suggest_params(nxs, params, &k, &maxdist) == -1 || lookup_enter(idx, "suggest", n, true) == -1) {
		return -1;
	}
	/* the filters a query token goes through (tokenizer.c:205-227): normalizer, stop words, stemmer */
	if (lookup_stage(idx, tokens, lens, n, ~0u, &st) == -1 || lookup_pack(nxs, &st, k) == -1) {
		goto out;
	}
	if (st.nd && nxsgpu_suggest(idx->dev, st.bytes, st.off, (uint32_t)st.nd, maxdist, k, st.ids, st.dist, st.df,
	    st.counts, st.matches) != 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "device suggest pass failed: %s", nxsgpu_last_error());
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		if (st.s[i].act != 0) {
			out[i] = lookup_build(idx, &st, i, &nd, k, st.dist, 0, "token", errs);
		} else if ((out[i] = sugg_build("", 0, true, 0, 0, NULL, NULL, NULL, NULL)) == NULL) {
			/* (the filters dropped the token: an object that says so) */
			if (errs) {
				errs[i] = NXS_ERR_SYSTEM;
			}
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		}
		failed += !out[i];
	}
	ret = failed;
out:
	lookup_free(&st);
	return ret;
}

int
nxs_index_suggest_batch(nxs_index_t *idx, nxs_params_t *params, const char *const *tokens, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	return suggest_run(idx, params, tokens, NULL, n, out, errs);
}

nxs_sugg_t *
nxs_index_suggest(nxs_index_t *idx, nxs_params_t *params, const char *token, size_t len)
{
	nxs_sugg_t *sg = NULL;

	/* (one string: the call fails exactly when it leaves no object) */
	(void)suggest_run(idx, params, &token, &len, 1, &sg, NULL);
	return sg;
}

/* ---- prefix completion (nxs_index_complete) ------------------------------------------- */

/* lens: NULL = the strings are NUL-terminated */
static int
complete_run(nxs_index_t *idx, nxs_params_t *params, const char *const *prefixes, const size_t *lens, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	lookup_t st = { 0 };
	unsigned k;
	size_t nd = 0;
	int ret = -1, failed = 0;

	nxs_clear_error(nxs);
	outs_clear(out, errs, n);
	if (get_limit_param(nxs, params, "complete_limit", &k) == -1 || lookup_enter(idx, "complete", n, true) == -1) {
		return -1;
	}
	/* a prefix is a fragment, not a word: the normalizer / lowercase stage only (nxs_filters_run_stages) */
	if (lookup_stage(idx, prefixes, lens, n, NXS_FSTAGE_NORMALIZER, &st) == -1) {
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		if (st.s[i].act == 1 && st.s[i].len == 0) {
			st.s[i].act = 0;		/* empty before or after normalisation: NXS_ERR_INVALID below */
		}
	}
	if (lookup_pack(nxs, &st, k) == -1) {
		goto out;
	}
	if (st.nd && nxsgpu_complete(idx->dev, st.bytes, st.off, (uint32_t)st.nd, k, st.ids, st.df, st.counts,
	    st.matches) != 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "device complete pass failed: %s", nxsgpu_last_error());
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		if (st.s[i].act != 0) {
			out[i] = lookup_build(idx, &st, i, &nd, k, NULL, st.s[i].len, "prefix", errs);
		} else {
			if (errs) {
				errs[i] = NXS_ERR_INVALID;
			}
			nxs_decl_err(nxs, NXS_ERR_INVALID, "empty prefix");
		}
		if (out[i]) {
			out[i]->kind = SUGG_COMPLETE;
		}
		failed += !out[i];
	}
	ret = failed;
out:
	lookup_free(&st);
	return ret;
}

int
nxs_index_complete_batch(nxs_index_t *idx, nxs_params_t *params, const char *const *prefixes, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	return complete_run(idx, params, prefixes, NULL, n, out, errs);
}

nxs_sugg_t *
nxs_index_complete(nxs_index_t *idx, nxs_params_t *params, const char *prefix, size_t len)
{
	nxs_sugg_t *sg = NULL;

	(void)complete_run(idx, params, &prefix, &len, 1, &sg, NULL);	/* (as nxs_index_suggest) */
	return sg;
}

/* ---- wildcard matching (nxs_index_wildcard) -------------------------------------------- */

/* lens: NULL = the strings are NUL-terminated */
static int
wildcard_run(nxs_index_t *idx, nxs_params_t *params, const char *const *patterns, const size_t *lens, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	lookup_t st = { 0 };
	size_t *lit = NULL;
	unsigned k;
	size_t nd = 0;
	int ret = -1, failed = 0;

	nxs_clear_error(nxs);
	outs_clear(out, errs, n);
	if (get_limit_param(nxs, params, "wildcard_limit", &k) == -1 || lookup_enter(idx, "wildcard", n, true) == -1) {
		return -1;
	}
	/* every literal piece through the normalizer / lowercase stage only, runs of stars collapsed
	 * (nxs_wild_normalize).  act: 1 = goes to the device, 0 = no literal byte, -1 = the filters failed,
	 * -3 = too long (-2: out of memory fails the call) */
	st.n = n;
	st.s = calloc(n ? n : 1, sizeof(*st.s));
	lit = calloc(n ? n : 1, sizeof(*lit));
	if (!st.s || !lit) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		st.s[i].act = nxs_wild_normalize(idx, patterns[i], lens ? lens[i] : strlen(patterns[i]), &st.s[i].val,
		    &st.s[i].len, &lit[i]);
		if (st.s[i].act == -2) {
			nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
			goto out;
		}
	}
	if (lookup_pack(nxs, &st, k) == -1) {
		goto out;
	}
	if (st.nd && nxsgpu_wildcard(idx->dev, st.bytes, st.off, (uint32_t)st.nd, k, st.ids, st.df, st.counts,
	    st.matches) != 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "device wildcard pass failed: %s", nxsgpu_last_error());
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		if (st.s[i].act == 1 || st.s[i].act == -1) {
			out[i] = lookup_build(idx, &st, i, &nd, k, NULL, lit[i], "pattern", errs);
		} else {
			if (errs) {
				errs[i] = NXS_ERR_INVALID;
			}
			nxs_decl_err(nxs, NXS_ERR_INVALID, st.s[i].act == 0 ? "empty pattern" : "wildcard pattern too long");
		}
		if (out[i]) {
			out[i]->kind = SUGG_WILD;
		}
		failed += !out[i];
	}
	ret = failed;
out:
	free(lit);
	lookup_free(&st);
	return ret;
}

int
nxs_index_wildcard_batch(nxs_index_t *idx, nxs_params_t *params, const char *const *patterns, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	return wildcard_run(idx, params, patterns, NULL, n, out, errs);
}

nxs_sugg_t *
nxs_index_wildcard(nxs_index_t *idx, nxs_params_t *params, const char *pattern, size_t len)
{
	nxs_sugg_t *sg = NULL;

	(void)wildcard_run(idx, params, &pattern, &len, 1, &sg, NULL);	/* (as nxs_index_suggest) */
	return sg;
}

/* ---- term vectors (nxs_index_doc_terms) -------------------------------------------------- */

/* `key`: a df floor (uint >= 1) */
static int
get_mindf_param(nxs_t *nxs, const nxs_params_t *params, const char *key, unsigned dflt, unsigned *mindf)
{
	uint64_t v;

	*mindf = dflt;
	if (params && nxs_params_get_uint(params, key, &v) == 0) {
		if (v < 1 || v > UINT32_MAX) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid %s (>= 1)", key);
			return -1;
		}
		*mindf = (unsigned)v;
	}
	return 0;
}

/* a term vector as the device reports it into an object; NULL: out of memory / an unknown term (declared) */
static nxs_sugg_t *
docterms_build(nxs_index_t *idx, uint64_t doc, uint64_t matches, unsigned count, const uint32_t *ids, const float *w,
    const uint32_t *tf, const uint32_t *df, nxs_err_t *code)
{
	const uint8_t *terms[NXS_SUGGEST_MAX] = { NULL };
	size_t tlens[NXS_SUGGEST_MAX] = { 0 };
	unsigned dists[NXS_SUGGEST_MAX] = { 0 };
	uint64_t dfs[NXS_SUGGEST_MAX] = { 0 };
	nxs_sugg_t *sg;

	for (unsigned j = 0; j < count; j++) {
		if (ids[j] < 1 || ids[j] > idx->last_id) {
			*code = NXS_ERR_FATAL;
			nxs_decl_err(idx->nxs, *code, "the device named an unknown term for doc %llu", (unsigned long long)doc);
			return NULL;
		}
		terms[j] = idx->terms[ids[j]].val;
		tlens[j] = idx->terms[ids[j]].len;
		dists[j] = tf[j];
		dfs[j] = df[j];
	}
	if ((sg = sugg_build("", 0, false, matches, count, terms, tlens, dists, dfs)) == NULL) {
		*code = NXS_ERR_SYSTEM;
		nxs_decl_err(idx->nxs, *code, "out of memory");
		return NULL;
	}
	sg->kind = SUGG_DOC;
	sg->doc_id = doc;
	for (unsigned j = 0; j < count; j++) {
		sg->items[j].score = w[j];
	}
	return sg;
}

int
docterms_rows(nxs_index_t *idx, int algo, const nxs_doc_id_t *docs, size_t n, unsigned mindf, unsigned k,
    docterms_rows_t *r)
{
	const size_t m = n ? n : 1;

	memset(r, 0, sizeof(*r));
	r->ids = malloc(m * k * sizeof(*r->ids));
	r->w = malloc(m * k * sizeof(*r->w));
	r->tf = malloc(m * k * sizeof(*r->tf));
	r->df = malloc(m * k * sizeof(*r->df));
	r->counts = malloc(m * sizeof(*r->counts));
	r->matches = malloc(m * sizeof(*r->matches));
	r->found = malloc(m);
	if (!r->ids || !r->w || !r->tf || !r->df || !r->counts || !r->matches || !r->found) {
		nxs_decl_err(idx->nxs, NXS_ERR_SYSTEM, "out of memory");
		docterms_rows_free(r);
		return -1;
	}
	if (nxsgpu_doc_terms(idx->dev, algo, docs, (uint32_t)n, mindf, k, r->ids, r->w, r->tf, r->df, r->counts, r->matches,
	    r->found) != 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_FATAL, "device doc_terms pass failed: %s", nxsgpu_last_error());
		docterms_rows_free(r);
		return -1;
	}
	for (size_t i = 0; i < n; i++) {
		r->found[i] = r->found[i] && nxs_index_doc_live(idx, docs[i]);
	}
	return 0;
}

void
docterms_rows_free(docterms_rows_t *r)
{
	free(r->ids);
	free(r->w);
	free(r->tf);
	free(r->df);
	free(r->counts);
	free(r->matches);
	free(r->found);
	memset(r, 0, sizeof(*r));
}

int
nxs_index_doc_terms_batch(nxs_index_t *idx, nxs_params_t *params, const nxs_doc_id_t *docs, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	search_params_t sp;
	docterms_rows_t r;
	unsigned k, mindf;
	int failed = 0;

	nxs_clear_error(nxs);
	outs_clear(out, errs, n);
	if (get_limit_param(nxs, params, "docterms_limit", &k) == -1 ||
	    get_mindf_param(nxs, params, "docterms_mindf", 1, &mindf) == -1 || get_search_params(idx, params, &sp) == -1 ||
	    lookup_enter(idx, "doc_terms", n, false) == -1) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	if (docterms_rows(idx, sp.algo, docs, n, mindf, k, &r) == -1) {
		return -1;
	}
	for (size_t i = 0; i < n; i++) {
		nxs_err_t code = NXS_ERR_MISSING;

		if (!r.found[i]) {
			nxs_decl_err(nxs, code, "no such document");
		} else {
			out[i] = docterms_build(idx, docs[i], r.matches[i], r.counts[i] <= k ? r.counts[i] : k, r.ids + i * k,
			    r.w + i * k, r.tf + i * k, r.df + i * k, &code);
		}
		if (!out[i]) {
			if (errs) {
				errs[i] = code;
			}
			failed++;
		}
	}
	docterms_rows_free(&r);
	return failed;
}

nxs_sugg_t *
nxs_index_doc_terms(nxs_index_t *idx, nxs_params_t *params, nxs_doc_id_t doc)
{
	nxs_sugg_t *sg = NULL;

	(void)nxs_index_doc_terms_batch(idx, params, &doc, 1, &sg, NULL);	/* (as nxs_index_suggest) */
	return sg;
}

/* ---- related terms (nxs_index_related) ---------------------------------------------------- */

/* related terms as the device reports them into an object; NULL: out of memory / an unknown term (declared) */
static nxs_sugg_t *
related_build(nxs_index_t *idx, const char *query, uint64_t docs, uint64_t matches, unsigned count, const uint32_t *ids,
    const uint32_t *c, const uint32_t *df, nxs_err_t *code)
{
	const uint8_t *terms[NXS_SUGGEST_MAX] = { NULL };
	size_t tlens[NXS_SUGGEST_MAX] = { 0 };
	unsigned dists[NXS_SUGGEST_MAX] = { 0 };
	uint64_t dfs[NXS_SUGGEST_MAX] = { 0 };
	nxs_sugg_t *sg;

	for (unsigned j = 0; j < count; j++) {
		if (ids[j] < 1 || ids[j] > idx->last_id || df[j] == 0) {
			*code = NXS_ERR_FATAL;
			nxs_decl_err(idx->nxs, *code, "the device named an unknown term for a related query");
			return NULL;
		}
		terms[j] = idx->terms[ids[j]].val;
		tlens[j] = idx->terms[ids[j]].len;
		dists[j] = c[j];
		dfs[j] = df[j];
	}
	if ((sg = sugg_build(query, strlen(query), false, matches, count, terms, tlens, dists, dfs)) == NULL) {
		*code = NXS_ERR_SYSTEM;
		nxs_decl_err(idx->nxs, *code, "out of memory");
		return NULL;
	}
	sg->kind = SUGG_RELATED;
	sg->docs = docs;
	for (unsigned j = 0; j < count; j++) {
		sg->items[j].score = nxs_rt_share(c[j], df[j]);
	}
	return sg;
}

/*
 * The front half is a search's (plan_batch: parse, filters, blocking fuzzy / prefix / wildcard resolution, truth
 * table or postfix program); the plan's resolved term ids are the exclusion list.  The fixed-size plans go to
 * nxsgpu_related in one call.
 */
int
nxs_index_related_batch(nxs_index_t *idx, nxs_params_t *params, const char *const *queries, size_t n,
    nxs_sugg_t **out, nxs_err_t *errs)
{
	nxs_t *nxs = idx->nxs;
	search_params_t sp;
	related_params_t rp;
	qprep_t *prep = NULL;
	nxsgpu_query_t *plans = NULL;
	uint32_t *rows = NULL, *slot = NULL;
	size_t np = 0;
	int ret = -1, failed = 0;

	nxs_clear_error(nxs);
	outs_clear(out, errs, n);
	if (get_related_params(nxs, params, &rp) == -1 || get_search_params(idx, params, &sp) == -1 ||
	    lookup_enter(idx, "related", n, false) == -1) {
		return -1;
	}
	if (n == 0) {
		return 0;
	}
	prep = calloc(n, sizeof(*prep));
	plans = malloc(n * sizeof(*plans));
	slot = malloc(n * sizeof(*slot));
	rows = malloc(n * (3 * (size_t)rp.k + 3) * sizeof(*rows));
	if (!prep || !plans || !slot || !rows) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		goto out;
	}
	if (plan_batch(idx, &sp, queries, NULL, n, prep) == -1) {
		goto out;
	}
	for (size_t i = 0; i < n; i++) {
		slot[i] = UINT32_MAX;
		if (!prep[i].errcode && !prep[i].wide && !prep[i].empty) {
			slot[i] = (uint32_t)np;
			plans[np++] = prep[i].plan;
		}
	}
	{
		uint32_t *ids = rows, *c = ids + np * rp.k, *df = c + np * rp.k, *counts = df + np * rp.k;
		uint32_t *matches = counts + np, *docs = matches + np;

		if (np && nxsgpu_related(idx->dev, sp.algo, plans, (uint32_t)np, rp.order, rp.mindf, rp.mincount, rp.self, rp.k,
		    ids, c, df, counts, matches, docs) != 0) {
			nxs_decl_err(nxs, NXS_ERR_FATAL, "device related pass failed: %s", nxsgpu_last_error());
			goto out;
		}
		for (size_t i = 0; i < n; i++) {
			nxs_err_t code = prep[i].errcode;
			const size_t s = slot[i];

			if (code) {
				/* what a search reports for the string */
				nxs_decl_err(nxs, code, "%s", prep[i].errmsg ? prep[i].errmsg : "");
			} else if (prep[i].wide) {
				code = NXS_ERR_LIMIT;
				nxs_decl_err(nxs, code, "related is not available for a query of more than %u terms", NXSGPU_MAX_TOKENS);
			} else if (s == UINT32_MAX) {
				/* resolves to nothing: an empty list */
				out[i] = related_build(idx, queries[i], 0, 0, 0, NULL, NULL, NULL, &code);
			} else {
				out[i] = related_build(idx, queries[i], docs[s], matches[s], counts[s] <= rp.k ? counts[s] : rp.k,
				    ids + s * rp.k, c + s * rp.k, df + s * rp.k, &code);
			}
			if (!out[i]) {
				if (errs) {
					errs[i] = code;
				}
				failed++;
			}
		}
	}
	ret = failed;
out:
	for (size_t i = 0; prep && i < n; i++) {
		nxs_query_release(&prep[i]);
	}
	free(prep);
	free(plans);
	free(slot);
	free(rows);
	return ret;
}

nxs_sugg_t *
nxs_index_related(nxs_index_t *idx, nxs_params_t *params, const char *query, size_t len)
{
	nxs_sugg_t *sg = NULL;

	(void)len;	/* (as nxs_index_search: the lexer stops at the NUL byte) */
	(void)nxs_index_related_batch(idx, params, &query, 1, &sg, NULL);	/* (as nxs_index_suggest) */
	return sg;
}

#ifdef NXS_TEST_HOOKS
/* the parameters as nxs_index_related reads its own keys: 0, or -1 with the error declared */
int
nxs_test_related_params(nxs_t *nxs, nxs_params_t *params, unsigned *k, int *order, unsigned *mindf, unsigned *mincount,
    int *self)
{
	related_params_t rp;

	nxs_clear_error(nxs);
	if (get_related_params(nxs, params, &rp) == -1) {
		return -1;
	}
	*k = rp.k;
	*order = rp.order;
	*mindf = rp.mindf;
	*mincount = rp.mincount;
	*self = rp.self;
	return 0;
}

/* an nxs_sugg_t of the related kind built by hand (the scores are the shares c / df) */
nxs_sugg_t *
nxs_test_related_build(const char *query, size_t query_len, uint64_t docs, uint64_t matches, unsigned count,
    const uint8_t *const *terms, const size_t *lens, const unsigned *cs, const uint64_t *dfs)
{
	nxs_sugg_t *sg = sugg_build(query, query_len, false, matches, count, terms, lens, cs, dfs);

	if (sg) {
		sg->kind = SUGG_RELATED;
		sg->docs = docs;
		for (unsigned i = 0; i < count; i++) {
			sg->items[i].score = nxs_rt_share(cs[i], (uint32_t)dfs[i]);
		}
	}
	return sg;
}
#endif /* NXS_TEST_HOOKS */

#ifdef NXS_TEST_HOOKS
/* the parameters as nxs_index_doc_terms / nxs_index_similar read them: 0, or -1 with the error declared */
int
nxs_test_docterms_params(nxs_t *nxs, nxs_params_t *params, unsigned *k, unsigned *mindf, unsigned *similar_terms,
    unsigned *similar_mindf, int *similar_self)
{
	nxs_index_t fake = { .nxs = nxs };
	search_params_t sp;

	nxs_clear_error(nxs);
	if (get_limit_param(nxs, params, "docterms_limit", k) == -1 ||
	    get_mindf_param(nxs, params, "docterms_mindf", 1, mindf) == -1 || get_search_params(&fake, params, &sp) == -1) {
		return -1;
	}
	*similar_terms = sp.similar_terms;
	*similar_mindf = sp.similar_mindf;
	*similar_self = sp.similar_self;
	return 0;
}

/* an nxs_sugg_t of the term-vector kind built by hand */
nxs_sugg_t *
nxs_test_docterms_build(uint64_t doc, uint64_t matches, unsigned count, const uint8_t *const *terms, const size_t *lens,
    const unsigned *tfs, const uint64_t *dfs, const float *scores)
{
	nxs_sugg_t *sg = sugg_build("", 0, false, matches, count, terms, lens, tfs, dfs);

	if (sg) {
		sg->kind = SUGG_DOC;
		sg->doc_id = doc;
		for (unsigned i = 0; i < count; i++) {
			sg->items[i].score = scores[i];
		}
	}
	return sg;
}
#endif /* NXS_TEST_HOOKS */

#ifdef NXS_TEST_HOOKS
/* the parameters as nxs_index_wildcard / a search read them: 0, or -1 with the error declared */
int
nxs_test_wild_params(nxs_t *nxs, nxs_params_t *params, unsigned *k, int *wildcardmatch, unsigned *wildcard_terms)
{
	nxs_index_t fake = { .nxs = nxs };
	search_params_t sp;

	nxs_clear_error(nxs);
	if (get_limit_param(nxs, params, "wildcard_limit", k) == -1 || get_search_params(&fake, params, &sp) == -1) {
		return -1;
	}
	*wildcardmatch = sp.wildcardmatch;
	*wildcard_terms = sp.wildcard_terms;
	return 0;
}

/* an nxs_sugg_t of the wildcard kind built by hand: distance = len(term) - the pattern's literal bytes */
nxs_sugg_t *
nxs_test_wild_build(const char *pattern, size_t pattern_len, uint64_t matches, unsigned count,
    const uint8_t *const *terms, const size_t *lens, const uint64_t *dfs)
{
	unsigned dists[NXS_SUGGEST_MAX];
	uint32_t lit, minlen;
	nxs_sugg_t *sg;

	(void)nxs_wild_shape((const uint8_t *)pattern, (uint32_t)pattern_len, &lit, &minlen);
	for (unsigned i = 0; i < count && i < NXS_SUGGEST_MAX; i++) {
		dists[i] = (unsigned)(lens[i] - lit);
	}
	if ((sg = sugg_build(pattern, pattern_len, false, matches, count, terms, lens, dists, dfs)) != NULL) {
		sg->kind = SUGG_WILD;
	}
	return sg;
}
#endif /* NXS_TEST_HOOKS */

#ifdef NXS_TEST_HOOKS
/* the parameters as nxs_index_complete / a search read them: 0, or -1 with the error declared */
int
nxs_test_complete_params(nxs_t *nxs, nxs_params_t *params, unsigned *k, int *prefixmatch, unsigned *prefix_limit)
{
	nxs_index_t fake = { .nxs = nxs };
	search_params_t sp;

	nxs_clear_error(nxs);
	if (get_limit_param(nxs, params, "complete_limit", k) == -1 || get_search_params(&fake, params, &sp) == -1) {
		return -1;
	}
	*prefixmatch = sp.prefixmatch;
	*prefix_limit = sp.prefix_limit;
	return 0;
}

/* an nxs_sugg_t of the completion kind built by hand */
nxs_sugg_t *
nxs_test_compl_build(const char *prefix, size_t prefix_len, uint64_t matches, unsigned count,
    const uint8_t *const *terms, const size_t *lens, const uint64_t *dfs)
{
	unsigned dists[NXS_SUGGEST_MAX];
	nxs_sugg_t *sg;

	for (unsigned i = 0; i < count && i < NXS_SUGGEST_MAX; i++) {
		dists[i] = (unsigned)(lens[i] - prefix_len);
	}
	if ((sg = sugg_build(prefix, prefix_len, false, matches, count, terms, lens, dists, dfs)) != NULL) {
		sg->kind = SUGG_COMPLETE;
	}
	return sg;
}

/* the parameters as nxs_index_suggest reads them: 0, or -1 with the error declared */
int
nxs_test_suggest_params(nxs_t *nxs, nxs_params_t *params, unsigned *k, unsigned *maxdist)
{
	nxs_clear_error(nxs);
	return get_suggest_params(nxs, params, k, maxdist);
}

/* an nxs_sugg_t built by hand (the accessors and the JSON writer without an index) */
nxs_sugg_t *
nxs_test_sugg_build(const char *token, size_t token_len, bool dropped, uint64_t matches, unsigned count,
    const uint8_t *const *terms, const size_t *lens, const unsigned *dists, const uint64_t *dfs)
{
	return sugg_build(token, token_len, dropped, matches, count, terms, lens, dists, dfs);
}
#endif /* NXS_TEST_HOOKS */
