/*
 * nxs_params.c -- nxs_params_t: the setters and getters, nxs_params_fromjson
 * and its JSON scanner, and the parameters a search reads.
 *   params                src/core/params.c
 *   search params         src/query/search.c:78-112  (limit / algo / fuzzymatch)
 */
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <limits.h>
#include <errno.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"

nxs_params_t *
nxs_params_create(void)
{
	return calloc(1, sizeof(nxs_params_t));
}

void
nxs_params_release(nxs_params_t *p)
{
	for (size_t i = 0; i < p->n; i++) {
		free(p->kv[i].key);
		free(p->kv[i].s);
	}
	free(p->kv);
	free(p);
}

static param_kv_t *
params_slot(nxs_params_t *p, const char *key)
{
	param_kv_t *kv;

	for (size_t i = 0; i < p->n; i++) {
		if (strcmp(p->kv[i].key, key) == 0) {
			free(p->kv[i].s);
			p->kv[i].s = NULL;
			return &p->kv[i];
		}
	}
	if ((kv = realloc(p->kv, (p->n + 1) * sizeof(param_kv_t))) == NULL) {
		return NULL;
	}
	p->kv = kv;
	kv = &p->kv[p->n++];
	memset(kv, 0, sizeof(*kv));
	kv->key = strdup(key);
	return kv;
}

int
nxs_params_set_str(nxs_params_t *p, const char *key, const char *val)
{
	param_kv_t *kv = params_slot(p, key);
	if (!kv) return -1;
	kv->type = PV_STR;
	kv->s = strdup(val);
	return 0;
}

int
nxs_params_set_uint(nxs_params_t *p, const char *key, uint64_t val)
{
	param_kv_t *kv = params_slot(p, key);
	if (!kv) return -1;
	kv->type = PV_UINT;
	kv->u = val;
	return 0;
}

int
nxs_params_set_bool(nxs_params_t *p, const char *key, bool val)
{
	param_kv_t *kv = params_slot(p, key);
	if (!kv) return -1;
	kv->type = PV_BOOL;
	kv->b = val;
	return 0;
}

static const param_kv_t *
params_find(const nxs_params_t *p, const char *key, pv_type_t type)
{
	for (size_t i = 0; p && i < p->n; i++) {
		if (strcmp(p->kv[i].key, key) == 0 && p->kv[i].type == type) {
			return &p->kv[i];
		}
	}
	return NULL;
}

const char *
nxs_params_get_str(const nxs_params_t *p, const char *key)
{
	const param_kv_t *kv = params_find(p, key, PV_STR);
	return kv ? kv->s : NULL;
}

int
nxs_params_get_uint(const nxs_params_t *p, const char *key, uint64_t *val)
{
	const param_kv_t *kv = params_find(p, key, PV_UINT);
	if (!kv) return -1;
	*val = kv->u;
	return 0;
}

int
nxs_params_get_bool(const nxs_params_t *p, const char *key, bool *val)
{
	const param_kv_t *kv = params_find(p, key, PV_BOOL);
	if (!kv) return -1;
	*val = kv->b;
	return 0;
}

/*
 * nxs_params_fromjson (params.c:201-208): how the reference's Lua / HTTP tier
 * hands `limit`, `algo` and `fuzzymatch` to nxs_index_search (lua.c:99-110).  The
 * reference parses with yyjson into a mutable document and the getters look a key
 * up in the ROOT OBJECT by type; here: a strict JSON scanner (RFC 8259, no
 * trailing content -- yyjson's default flags) that keeps the root object's
 * string / unsigned-integer / bool members and validates and skips everything
 * else (negative or fractional numbers, null, arrays, nested objects: no getter of
 * the query path reads those).  A syntax error is NXS_ERR_SYSTEM "params parsing
 * failed: ... at <offset>", as there.
 */
typedef struct {
	const char *	p;
	const char *	end;
	const char *	beg;
	const char *	err;
} jscan_t;

static void
js_ws(jscan_t *j)
{
	while (j->p < j->end && (*j->p == ' ' || *j->p == '\t' || *j->p == '\n' || *j->p == '\r')) {
		j->p++;
	}
}

static int
js_fail(jscan_t *j, const char *msg)
{
	if (!j->err) {
		j->err = msg;
	}
	return -1;
}

static int
js_hex4(jscan_t *j, unsigned *out)
{
	unsigned v = 0;

	if (j->end - j->p < 4) {
		return js_fail(j, "invalid escaped sequence in string");
	}
	for (int i = 0; i < 4; i++) {
		const char c = *j->p++;
		v <<= 4;
		if (c >= '0' && c <= '9') v |= (unsigned)(c - '0');
		else if (c >= 'a' && c <= 'f') v |= (unsigned)(c - 'a' + 10);
		else if (c >= 'A' && c <= 'F') v |= (unsigned)(c - 'A' + 10);
		else return js_fail(j, "invalid escaped sequence in string");
	}
	*out = v;
	return 0;
}

/* a string; *out (if wanted) = malloc'ed, unescaped, NUL-terminated copy */
static int
js_string(jscan_t *j, char **out)
{
	char *buf = NULL;
	size_t n = 0;

	if (j->p >= j->end || *j->p != '"') {
		return js_fail(j, "unexpected character");
	}
	j->p++;
	if (out && (buf = malloc((size_t)(j->end - j->p) + 1)) == NULL) {
		return js_fail(j, "out of memory");
	}
	while (j->p < j->end && *j->p != '"') {
		unsigned char c = (unsigned char)*j->p++;

		if (c < 0x20) {
			free(buf);
			return js_fail(j, "unexpected control character in string");
		}
		if (c == '\\') {
			unsigned cp;

			if (j->p >= j->end) {
				break;
			}
			c = (unsigned char)*j->p++;
			switch (c) {
			case '"': case '\\': case '/': cp = c; break;
			case 'b': cp = '\b'; break;
			case 'f': cp = '\f'; break;
			case 'n': cp = '\n'; break;
			case 'r': cp = '\r'; break;
			case 't': cp = '\t'; break;
			case 'u':
				if (js_hex4(j, &cp) == -1) {
					free(buf);
					return -1;
				}
				if (cp >= 0xd800 && cp <= 0xdbff) {	/* surrogate pair */
					unsigned lo;
					if (j->end - j->p < 6 || j->p[0] != '\\' || j->p[1] != 'u') {
						free(buf);
						return js_fail(j, "no low surrogate in string");
					}
					j->p += 2;
					if (js_hex4(j, &lo) == -1 || lo < 0xdc00 || lo > 0xdfff) {
						free(buf);
						return js_fail(j, "invalid low surrogate in string");
					}
					cp = 0x10000 + ((cp - 0xd800) << 10) + (lo - 0xdc00);
				} else if (cp >= 0xdc00 && cp <= 0xdfff) {
					free(buf);
					return js_fail(j, "invalid high surrogate in string");
				}
				break;
			default:
				free(buf);
				return js_fail(j, "invalid escaped character in string");
			}
			if (buf) {
				if (cp < 0x80) {
					buf[n++] = (char)cp;
				} else if (cp < 0x800) {
					buf[n++] = (char)(0xc0 | (cp >> 6));
					buf[n++] = (char)(0x80 | (cp & 0x3f));
				} else if (cp < 0x10000) {
					buf[n++] = (char)(0xe0 | (cp >> 12));
					buf[n++] = (char)(0x80 | ((cp >> 6) & 0x3f));
					buf[n++] = (char)(0x80 | (cp & 0x3f));
				} else {
					buf[n++] = (char)(0xf0 | (cp >> 18));
					buf[n++] = (char)(0x80 | ((cp >> 12) & 0x3f));
					buf[n++] = (char)(0x80 | ((cp >> 6) & 0x3f));
					buf[n++] = (char)(0x80 | (cp & 0x3f));
				}
			}
			continue;
		}
		if (buf) {
			buf[n++] = (char)c;
		}
	}
	if (j->p >= j->end) {
		free(buf);
		return js_fail(j, "unclosed string");
	}
	j->p++;		/* the closing quote */
	if (buf) {
		buf[n] = '\0';
		*out = buf;
	}
	return 0;
}

/* a number; *is_uint: a non-negative integer without fraction / exponent that fits u64 */
static int
js_number(jscan_t *j, bool *is_uint, uint64_t *u)
{
	const char *s = j->p;
	bool neg = false, integral = true, fits = true;
	uint64_t v = 0;

	if (j->p < j->end && *j->p == '-') {
		neg = true;
		j->p++;
	}
	if (j->p >= j->end || *j->p < '0' || *j->p > '9') {
		j->p = s;
		return js_fail(j, "unexpected character");
	}
	if (*j->p == '0') {
		j->p++;
		if (j->p < j->end && *j->p >= '0' && *j->p <= '9') {
			return js_fail(j, "number with leading zero is not allowed");
		}
	} else {
		while (j->p < j->end && *j->p >= '0' && *j->p <= '9') {
			const unsigned d = (unsigned)(*j->p++ - '0');
			if (v > (UINT64_MAX - d) / 10) {
				fits = false;
			} else {
				v = v * 10 + d;
			}
		}
	}
	if (j->p < j->end && *j->p == '.') {
		integral = false;
		j->p++;
		if (j->p >= j->end || *j->p < '0' || *j->p > '9') {
			return js_fail(j, "no digit after decimal point");
		}
		while (j->p < j->end && *j->p >= '0' && *j->p <= '9') {
			j->p++;
		}
	}
	if (j->p < j->end && (*j->p == 'e' || *j->p == 'E')) {
		integral = false;
		j->p++;
		if (j->p < j->end && (*j->p == '+' || *j->p == '-')) {
			j->p++;
		}
		if (j->p >= j->end || *j->p < '0' || *j->p > '9') {
			return js_fail(j, "no digit after exponent sign");
		}
		while (j->p < j->end && *j->p >= '0' && *j->p <= '9') {
			j->p++;
		}
	}
	*is_uint = !neg && integral && fits;
	*u = v;
	return 0;
}

static int js_value(jscan_t *j, nxs_params_t *into, const char *key, unsigned depth);

static int
js_literal(jscan_t *j, const char *word)
{
	const size_t n = strlen(word);

	if ((size_t)(j->end - j->p) < n || memcmp(j->p, word, n) != 0) {
		return js_fail(j, "invalid literal");
	}
	j->p += n;
	return 0;
}

/* one value; if `into` (the root object's member `key`), keep what the getters read */
static int
js_value(jscan_t *j, nxs_params_t *into, const char *key, unsigned depth)
{
	js_ws(j);
	if (j->p >= j->end) {
		return js_fail(j, "unexpected end of data");
	}
	if (depth > 512) {
		return js_fail(j, "nesting too deep");
	}
	switch (*j->p) {
	case '"': {
		char *str = NULL;

		if (js_string(j, into ? &str : NULL) == -1) {
			return -1;
		}
		if (into) {
			const int r = nxs_params_set_str(into, key, str);
			free(str);
			return r == 0 ? 0 : js_fail(j, "out of memory");
		}
		return 0;
	}
	case 't':
		if (js_literal(j, "true") == -1) return -1;
		return into && nxs_params_set_bool(into, key, true) != 0 ? js_fail(j, "out of memory") : 0;
	case 'f':
		if (js_literal(j, "false") == -1) return -1;
		return into && nxs_params_set_bool(into, key, false) != 0 ? js_fail(j, "out of memory") : 0;
	case 'n':
		return js_literal(j, "null");
	case '[':
		j->p++;
		js_ws(j);
		if (j->p < j->end && *j->p == ']') {
			j->p++;
			return 0;
		}
		for (;;) {
			if (js_value(j, NULL, NULL, depth + 1) == -1) {
				return -1;
			}
			js_ws(j);
			if (j->p < j->end && *j->p == ',') {
				j->p++;
				continue;
			}
			if (j->p < j->end && *j->p == ']') {
				j->p++;
				return 0;
			}
			return js_fail(j, j->p < j->end ? "unexpected character" : "unclosed array");
		}
	case '{': {
		/* only the ROOT object's members are parameters */
		nxs_params_t *const members = (depth == 0) ? into : NULL;

		j->p++;
		js_ws(j);
		if (j->p < j->end && *j->p == '}') {
			j->p++;
			return 0;
		}
		for (;;) {
			char *k = NULL;
			int r;

			js_ws(j);
			if (js_string(j, &k) == -1) {
				return -1;
			}
			js_ws(j);
			if (j->p >= j->end || *j->p != ':') {
				free(k);
				return js_fail(j, "unexpected character");
			}
			j->p++;
			/* (an embedded NUL would truncate the key: such a key is no parameter) */
			/*
			 * The reference's getters look a key up with yyjson_mut_obj_get(): the FIRST
			 * member of that name, whatever its kind -- a later duplicate is never seen,
			 * and a first member of a kind the getter does not read (null, a negative
			 * number, an array ...) hides a later usable one.  So only the first
			 * occurrence is kept, as a typeless entry if need be.
			 */
			{
				nxs_params_t *dst = members;
				bool first = false;

				if (members && k) {
					first = true;
					for (size_t i = 0; i < members->n; i++) {
						if (strcmp(members->kv[i].key, k) == 0) {
							first = false;
							break;
						}
					}
					if (!first) {
						dst = NULL;
					}
				}
				const size_t n_before = members ? members->n : 0;
				r = js_value(j, dst, k, depth + 1);
				if (r == 0 && first && members->n == n_before) {
					param_kv_t *kv = params_slot(members, k);
					if (!kv) {
						r = js_fail(j, "out of memory");
					} else {
						kv->type = PV_NONE;
					}
				}
			}
			free(k);
			if (r == -1) {
				return -1;
			}
			js_ws(j);
			if (j->p < j->end && *j->p == ',') {
				j->p++;
				continue;
			}
			if (j->p < j->end && *j->p == '}') {
				j->p++;
				return 0;
			}
			return js_fail(j, j->p < j->end ? "unexpected character" : "unclosed object");
		}
	}
	default: {
		bool is_uint = false;
		uint64_t u = 0;

		if (js_number(j, &is_uint, &u) == -1) {
			return -1;
		}
		if (into && is_uint && nxs_params_set_uint(into, key, u) != 0) {
			return js_fail(j, "out of memory");
		}
		return 0;
	}
	}
}

nxs_params_t *
nxs_params_fromjson(nxs_t *nxs, const char *json, size_t len)
{
	nxs_params_t *params;
	jscan_t j = { json, json + len, json, NULL };

	if ((params = nxs_params_create()) == NULL) {
		return NULL;
	}
	/* the root: its members if it is an object, nothing otherwise (the getters
	 * look keys up in the root object) */
	js_ws(&j);
	if (j.p < j.end && *j.p == '{') {
		if (js_value(&j, params, NULL, 0) == -1) {
			goto fail;
		}
	} else if (js_value(&j, NULL, NULL, 1) == -1) {
		goto fail;
	}
	js_ws(&j);
	if (j.p < j.end) {
		js_fail(&j, "unexpected content after document");
		goto fail;
	}
	return params;
fail:
	nxs_params_release(params);
	nxs_decl_err(nxs, NXS_ERR_SYSTEM, "params parsing failed: %s at %u",
	    j.err ? j.err : "invalid JSON", (unsigned)(j.p - j.beg));
	return NULL;
}

/* ranking.c:182-192 */
int
get_ranking_func_id(const char *name)
{
	if (strcasecmp(name, "TF-IDF") == 0) {
		return NXSGPU_TF_IDF;
	}
	if (strcasecmp(name, "BM25") == 0) {
		return NXSGPU_BM25;
	}
	return -1;
}

/* ---- search -------------------------------------------------------------------- */

/* get_search_params: search.c:78-112 */
int
get_search_params(nxs_index_t *idx, nxs_params_t *params, search_params_t *sp)
{
	const char *s;
	uint64_t v;
	bool fl;

	sp->limit = NXS_DEFAULT_RESULTS_LIMIT;
	sp->fuzzymatch = true;
	sp->total = false;
	sp->prefixmatch = false;
	sp->prefix_limit = 8;
	sp->wildcardmatch = false;
	sp->wildcard_terms = 8;
	sp->explain = false;
	sp->similar_terms = 8;
	sp->similar_mindf = 2;
	sp->similar_self = false;
	sp->algo = idx->algo;
	if (!params) {
		return 0;
	}
	if (nxs_params_get_uint(params, "limit", &sp->limit) == 0 &&
	    (sp->limit == 0 || sp->limit > UINT_MAX)) {
		nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "invalid limit");
		return -1;
	}
	if ((s = nxs_params_get_str(params, "algo")) != NULL &&
	    (sp->algo = get_ranking_func_id(s)) < 0) {
		nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "invalid algorithm");
		return -1;
	}
	if (nxs_params_get_bool(params, "fuzzymatch", &fl) == 0 && !fl) {
		sp->fuzzymatch = false;
	}
	if (nxs_params_get_bool(params, "total", &fl) == 0 && fl) {
		sp->total = true;
	}
	if (nxs_params_get_bool(params, "prefixmatch", &fl) == 0 && fl) {
		sp->prefixmatch = true;
	}
	if (nxs_params_get_bool(params, "explain", &fl) == 0 && fl) {
		sp->explain = true;
	}
	if (nxs_params_get_uint(params, "prefix_limit", &v) == 0) {
		if (v < 1 || v > NXS_PREFIX_MAX) {
			nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "invalid prefix_limit (1..%d)", NXS_PREFIX_MAX);
			return -1;
		}
		sp->prefix_limit = (unsigned)v;
	}
	if (nxs_params_get_bool(params, "wildcardmatch", &fl) == 0 && fl) {
		sp->wildcardmatch = true;
	}
	if (nxs_params_get_uint(params, "wildcard_terms", &v) == 0) {
		if (v < 1 || v > NXS_PREFIX_MAX) {
			nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "invalid wildcard_terms (1..%d)", NXS_PREFIX_MAX);
			return -1;
		}
		sp->wildcard_terms = (unsigned)v;
	}
	if (nxs_params_get_uint(params, "similar_terms", &v) == 0) {
		if (v < 1 || v > NXS_PREFIX_MAX) {
			nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "invalid similar_terms (1..%d)", NXS_PREFIX_MAX);
			return -1;
		}
		sp->similar_terms = (unsigned)v;
	}
	if (nxs_params_get_uint(params, "similar_mindf", &v) == 0) {
		if (v < 1 || v > UINT32_MAX) {
			nxs_decl_err(idx->nxs, NXS_ERR_INVALID, "invalid similar_mindf (>= 1)");
			return -1;
		}
		sp->similar_mindf = (unsigned)v;
	}
	if (nxs_params_get_bool(params, "similar_self", &fl) == 0 && fl) {
		sp->similar_self = true;
	}
	return 0;
}

#ifdef NXS_TEST_HOOKS
/* explanations: the "explain" key as a search reads it (0, or -1 with the error declared) */
int
nxs_test_explain_params(nxs_t *nxs, nxs_params_t *params, int *explain)
{
	nxs_index_t fake = { .nxs = nxs };
	search_params_t sp;

	nxs_clear_error(nxs);
	if (get_search_params(&fake, params, &sp) == -1) {
		return -1;
	}
	*explain = sp.explain;
	return 0;
}
#endif /* NXS_TEST_HOOKS */

/*
 * The parameters of nxs_index_related, validated as the docterms_* keys are: "related_limit" (uint,
 * 1..NXS_SUGGEST_MAX, default 5), "related_order" ("count", the default, or "share"), "related_mindf" and
 * "related_mincount" (uint >= 1, default 1), "related_self" (bool, default false).  0, or -1 with
 * NXS_ERR_INVALID and a message that names the key.
 */
int
get_related_params(nxs_t *nxs, const nxs_params_t *params, related_params_t *rp)
{
	static const char *const floors[] = { "related_mindf", "related_mincount" };
	unsigned *const floor_of[] = { &rp->mindf, &rp->mincount };
	const char *s;
	uint64_t v;
	bool fl;

	rp->k = 5;
	rp->order = NXS_RT_COUNT;
	rp->mindf = 1;
	rp->mincount = 1;
	rp->self = false;
	if (!params) {
		return 0;
	}
	if (nxs_params_get_uint(params, "related_limit", &v) == 0) {
		if (v < 1 || v > NXS_SUGGEST_MAX) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid related_limit (1..%d)", NXS_SUGGEST_MAX);
			return -1;
		}
		rp->k = (unsigned)v;
	}
	for (int i = 0; i < 2; i++) {
		if (nxs_params_get_uint(params, floors[i], &v) == 0) {
			if (v < 1 || v > UINT32_MAX) {
				nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid %s (>= 1)", floors[i]);
				return -1;
			}
			*floor_of[i] = (unsigned)v;
		}
	}
	if ((s = nxs_params_get_str(params, "related_order")) != NULL) {
		if (strcmp(s, "count") == 0) {
			rp->order = NXS_RT_COUNT;
		} else if (strcmp(s, "share") == 0) {
			rp->order = NXS_RT_SHARE;
		} else {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid related_order (\"count\" or \"share\")");
			return -1;
		}
	}
	if (nxs_params_get_bool(params, "related_self", &fl) == 0 && fl) {
		rp->self = true;
	}
	return 0;
}

/*
 * The parameters of nxs_index_match_docs, validated as the related_* keys are: "match_limit" (uint,
 * 1..NXS_MATCH_MAX, default 1000) and "match_from" (uint, default 0: any doc id is a cursor).  0, or -1 with
 * NXS_ERR_INVALID and a message that names the key.
 */
int
get_match_params(nxs_t *nxs, const nxs_params_t *params, match_params_t *mp)
{
	uint64_t v;

	mp->limit = 1000;
	mp->from = 0;
	if (!params) {
		return 0;
	}
	if (nxs_params_get_uint(params, "match_limit", &v) == 0) {
		if (v < 1 || v > NXS_MATCH_MAX) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid match_limit (1..%u)", NXS_MATCH_MAX);
			return -1;
		}
		mp->limit = (unsigned)v;
	}
	if (nxs_params_get_uint(params, "match_from", &v) == 0) {
		mp->from = v;
	}
	return 0;
}
