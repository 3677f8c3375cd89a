/*
 * nxs_api.c -- the public C API (include/nxs.h): library instance and error
 * slot, index open/close.  The other subsystems of the host side have a unit
 * each (nxs_api_int.h maps them).
 *
 * Mirrors the reference's conventions for this path:
 *   error slot            src/core/nxs.c:154-217, nxs_impl.h:84-90
 *   index open            src/core/nxs.c:236-330
 * All scoring, boolean filtering, top-k and fuzzy matching run on the GPU
 * through include/nxs_gpu.h; there is no CPU fallback: without a HIP device
 * nxs_index_open() fails.
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>
#include <string.h>
#include <errno.h>
#include <sys/stat.h>

#include "nxs_api_int.h"
#include "nxs_hooks.h"

/* ---- instance + errors --------------------------------------------------- */

nxs_t *
nxs_open(const char *basedir)
{
	nxs_t *nxs = calloc(1, sizeof(nxs_t));
	const char *s = basedir ? basedir : getenv("NXS_BASEDIR");	/* nxs.c:109 */

	if (!nxs) {
		return NULL;
	}
	if (s == NULL || (nxs->basedir = realpath(s, NULL)) == NULL) {
		free(nxs);
		return NULL;
	}
	return nxs;
}

void
nxs_close(nxs_t *nxs)
{
	while (nxs->n_indexes) {
		nxs_index_close(nxs->indexes[nxs->n_indexes - 1]);
	}
	pool_destroy(nxs->pool);
	free(nxs->indexes);
	free(nxs->basedir);
	free(nxs->errmsg);
	free(nxs);
}

void
nxs_clear_error(nxs_t *nxs)
{
	free(nxs->errmsg);
	nxs->errmsg = NULL;
	nxs->errcode = NXS_ERR_SUCCESS;
}

void
nxs_decl_err(nxs_t *nxs, nxs_err_t code, const char *fmt, ...)
{
	char *msg = NULL;
	va_list ap;

	va_start(ap, fmt);
	if (vasprintf(&msg, fmt, ap) == -1) {
		msg = NULL;
	}
	va_end(ap);
	free(nxs->errmsg);
	nxs->errmsg = msg;
	nxs->errcode = code;
}

nxs_err_t
nxs_get_error(const nxs_t *nxs, const char **errmsg)
{
	if (errmsg) {
		*errmsg = nxs->errmsg;
	}
	return nxs->errcode;
}

/* ---- index open / close ---------------------------------------------------- */

/* str_isalnumdu(): index names are [A-Za-z0-9_-]+ (nxs.c:236-240) */
static bool
name_ok(const char *s)
{
	if (!*s) {
		return false;
	}
	for (; *s; s++) {
		const char c = *s;
		if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') ||
		    (c >= '0' && c <= '9') || c == '-' || c == '_')) {
			return false;
		}
	}
	return true;
}

static nxs_index_t *
index_open_common(nxs_t *nxs, const char *name, const char *terms_path,
    const char *dtmap_path, int algo, const char *const *filters, size_t n_filters,
    const char *lang)
{
	nxs_index_t *idx = calloc(1, sizeof(nxs_index_t)), **list;
	const char *ferr = NULL;

	if (!idx) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		return NULL;
	}
	idx->nxs = nxs;
	idx->algo = algo;
	idx->name = strdup(name);
	/* filter_pipeline_create (nxs.c:412-419): the query side of it */
	if (n_filters) {
		idx->filters = nxs_filters_create(nxs->basedir, filters, n_filters, lang, &ferr);
		if (!idx->filters) {
			nxs_decl_err(nxs, NXS_ERR_INVALID, "%s", ferr ? ferr : "filter pipeline failed");
			free(idx->name);
			free(idx);
			return NULL;
		}
		for (size_t i = 0; i < n_filters; i++) {
			idx->lowercase = idx->lowercase || strcmp(filters[i], "normalizer") == 0;
		}
	}
	if (nxs_index_load(idx, terms_path, dtmap_path) == -1) {
		nxs_index_unload(idx);
		nxs_filters_destroy(idx->filters);
		free(idx->name);
		free(idx);
		return NULL;
	}
	list = realloc(nxs->indexes, (nxs->n_indexes + 1) * sizeof(void *));
	nxs->indexes = list;
	nxs->indexes[nxs->n_indexes++] = idx;
	return idx;
}

/* minimal reader for the JSON params.db the reference writes (nxs.c:282-288) */
static char *
json_get_str(const char *json, const char *key)
{
	char pat[64];
	const char *p, *e;

	snprintf(pat, sizeof(pat), "\"%s\"", key);
	if ((p = strstr(json, pat)) == NULL) {
		return NULL;
	}
	p += strlen(pat);
	while (*p == ' ' || *p == ':' || *p == '\t' || *p == '\n') p++;
	if (*p != '"') {
		return NULL;
	}
	p++;
	if ((e = strchr(p, '"')) == NULL) {
		return NULL;
	}
	return strndup(p, e - p);
}

/* the strings of a JSON array of strings: "key": ["a", "b"] -> count */
static size_t
json_get_strlist(const char *json, const char *key, char **out, size_t cap)
{
	char pat[64];
	const char *p, *end;
	size_t n = 0;

	snprintf(pat, sizeof(pat), "\"%s\"", key);
	if ((p = strstr(json, pat)) == NULL) {
		return 0;
	}
	p += strlen(pat);
	while (*p == ' ' || *p == ':' || *p == '\t' || *p == '\n') p++;
	if (*p != '[' || (end = strchr(p, ']')) == NULL) {
		return 0;
	}
	while (n < cap) {
		const char *q = memchr(p, '"', (size_t)(end - p)), *e;
		if (!q || (e = memchr(q + 1, '"', (size_t)(end - q - 1))) == NULL) {
			break;
		}
		out[n++] = strndup(q + 1, (size_t)(e - q - 1));
		p = e + 1;
	}
	return n;
}

nxs_index_t *
nxs_index_open(nxs_t *nxs, const char *name)
{
	char *ppath = NULL, *tpath = NULL, *dpath = NULL, *json = NULL, *algo_name = NULL;
	char *filters[8] = { NULL }, *lang = NULL;
	size_t n_filters = 0;
	nxs_index_t *idx = NULL;
	struct stat sb;
	FILE *fp;
	int algo;

	nxs_clear_error(nxs);
	if (!name_ok(name)) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid characters in index name");
		return NULL;
	}
	for (size_t i = 0; i < nxs->n_indexes; i++) {
		if (strcmp(nxs->indexes[i]->name, name) == 0) {
			nxs_decl_err(nxs, NXS_ERR_EXISTS, "index `%s' is already open", name);
			return NULL;
		}
	}
	if (asprintf(&ppath, "%s/data/%s/params.db", nxs->basedir, name) == -1 ||
	    asprintf(&tpath, "%s/data/%s/nxsterms", nxs->basedir, name) == -1 ||
	    asprintf(&dpath, "%s/data/%s/nxsdtmap", nxs->basedir, name) == -1) {
		goto out;
	}
	if (stat(ppath, &sb) == -1 && errno == ENOENT) {
		nxs_decl_err(nxs, NXS_ERR_MISSING, "index `%s' does not exist", name);
		goto out;
	}
	if ((fp = fopen(ppath, "r")) == NULL) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "could not open %s: %s", ppath, strerror(errno));
		goto out;
	}
	json = calloc(1, sb.st_size + 1);
	if (fread(json, 1, sb.st_size, fp) != (size_t)sb.st_size) {
		fclose(fp);
		nxs_decl_err(nxs, NXS_ERR_FATAL, "corrupted index params");
		goto out;
	}
	fclose(fp);
	if ((algo_name = json_get_str(json, "algo")) == NULL) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "corrupted index params");	/* nxs.c:405-409 */
		goto out;
	}
	algo = get_ranking_func_id(algo_name);
	if (algo < 0) {
		nxs_decl_err(nxs, NXS_ERR_FATAL, "corrupted index params");
		goto out;
	}
	/* "filters": [...] in list order, "lang" (nxs.c:263-266; params.db) */
	n_filters = json_get_strlist(json, "filters", filters, 8);
	lang = json_get_str(json, "lang");
	idx = index_open_common(nxs, name, tpath, dpath, algo,
	    (const char *const *)filters, n_filters, lang);
out:
	for (size_t i = 0; i < n_filters; i++) {
		free(filters[i]);
	}
	free(lang);
	free(ppath);
	free(tpath);
	free(dpath);
	free(json);
	free(algo_name);
	return idx;
}

nxs_index_t *
nxs_index_open_files(nxs_t *nxs, const char *terms_path, const char *dtmap_path,
    const char *algo_name, bool lowercase)
{
	const int algo = get_ranking_func_id(algo_name ? algo_name : "BM25");

	nxs_clear_error(nxs);
	if (algo < 0) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "invalid algorithm");
		return NULL;
	}
	{
		static const char *const norm_only[] = { "normalizer" };
		return index_open_common(nxs, terms_path, terms_path, dtmap_path, algo,
		    norm_only, lowercase ? 1 : 0, "en");
	}
}

/* N4: one shard of a doc-sharded collection (include/nxs.h) */
nxs_index_t *
nxs_index_open_shard(nxs_t *nxs, const char *terms_path, const char *dtmap_path,
    const char *algo_name, bool lowercase, unsigned shard, unsigned n_shards, int device)
{
	static const char *const norm_only[] = { "normalizer" };
	const int algo = get_ranking_func_id(algo_name ? algo_name : "BM25");
	nxs_index_t *idx, **list;
	const char *ferr = NULL;

	nxs_clear_error(nxs);
	if (algo < 0 || n_shards == 0 || shard >= n_shards) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, algo < 0 ? "invalid algorithm" : "invalid shard");
		return NULL;
	}
	if ((idx = calloc(1, sizeof(nxs_index_t))) == NULL) {
		nxs_decl_err(nxs, NXS_ERR_SYSTEM, "out of memory");
		return NULL;
	}
	idx->nxs = nxs;
	idx->algo = algo;
	idx->lowercase = lowercase;
	idx->shard = shard;
	idx->n_shards = n_shards;
	idx->want_device = device >= 0 ? device + 1 : 0;
	idx->name = strdup(terms_path);
	if (lowercase && (idx->filters = nxs_filters_create(nxs->basedir, norm_only, 1, "en", &ferr)) == NULL) {
		nxs_decl_err(nxs, NXS_ERR_INVALID, "%s", ferr ? ferr : "filter pipeline failed");
		free(idx->name);
		free(idx);
		return NULL;
	}
	if (nxs_index_load(idx, terms_path, dtmap_path) == -1) {
		nxs_index_unload(idx);
		nxs_filters_destroy(idx->filters);
		free(idx->name);
		free(idx);
		return NULL;
	}
	list = realloc(nxs->indexes, (nxs->n_indexes + 1) * sizeof(void *));
	nxs->indexes = list;
	nxs->indexes[nxs->n_indexes++] = idx;
	return idx;
}

void
nxs_index_close(nxs_index_t *idx)
{
	nxs_t *nxs = idx->nxs;

	for (size_t i = 0; i < nxs->n_indexes; i++) {
		if (nxs->indexes[i] == idx) {
			nxs->indexes[i] = nxs->indexes[--nxs->n_indexes];
			break;
		}
	}
	index_drain(idx);
	if (idx->comm) {
		if (idx->dev) {
			(void)nxsgpu_index_set_comm(idx->dev, NULL);
		}
		nxsgpu_comm_destroy(idx->comm);
		idx->comm = NULL;
	}
	free(idx->emu_block);
	nxs_filters_destroy(idx->filters);
	nxs_index_unload(idx);
	plan_cache_destroy(idx->pcache);
	free(idx->name);
	free(idx);
}

#ifdef NXS_TEST_HOOKS
struct nxsgpu_index *
nxs_index_device(nxs_index_t *idx)
{
	return idx->dev;
}

/* bench: plan cache on / off at run time (the environment decides it otherwise, once) */
void
nxs_index_set_plan_cache(nxs_index_t *idx, int on)
{
	extern void nxs_plan_cache_switch(nxs_index_t *, int);
	nxs_plan_cache_switch(idx, on);
}
#endif
