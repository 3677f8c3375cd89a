/*
 * nxs_impl.h -- private declarations of the C11 host side: what nxs_index.c,
 * nxs_query.c and nxs_filters.c share with the units of the public API (those
 * have nxs_api_int.h among themselves).
 *
 * Host responsibilities (everything that is not per-posting or per-BK-node
 * work): mapping and validating the two index files, the term dictionary,
 * building and flattening the BK-tree image, query lexing/parsing, token
 * resolution, compiling a query into the device plan, and the nxs_resp_t
 * object.  All per-posting and per-node work happens on the device, in the
 * nxs_gpu_*.hip units (nxs_gpu_int.h maps them).
 */
#ifndef NXS_IMPL_H
#define NXS_IMPL_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#include "nxs.h"
#include "nxs_gpu.h"

#define	NXS_DEFAULT_RESULTS_LIMIT	1000	/* nxs_impl.h:39 of the reference */
#define	NXS_QUERY_RLIMIT		100	/* search.c:70 */
#define	LEVDIST_TOLERANCE		2	/* index.h:26 */

struct nxs_pool;

struct nxs {
	char *		basedir;
	char *		errmsg;
	nxs_err_t	errcode;
	nxs_index_t **	indexes;
	size_t		n_indexes;
	struct nxs_pool *pool;		/* host workers of the batch front half */
	bool		pool_tried;
};

void	nxs_clear_error(nxs_t *);
void	nxs_decl_err(nxs_t *, nxs_err_t, const char *fmt, ...)
	    __attribute__((format(printf, 3, 4)));

/* ---- params ---------------------------------------------------------- */

typedef enum { PV_STR, PV_UINT, PV_BOOL, PV_NONE } pv_type_t;	/* PV_NONE: a JSON member of a kind no getter reads */

typedef struct {
	char *		key;
	pv_type_t	type;
	char *		s;
	uint64_t	u;
	bool		b;
} param_kv_t;

struct nxs_params {
	param_kv_t *	kv;
	size_t		n;
};

const char *nxs_params_get_str(const nxs_params_t *, const char *);
int	nxs_params_get_uint(const nxs_params_t *, const char *, uint64_t *);
int	nxs_params_get_bool(const nxs_params_t *, const char *, bool *);

/* ---- index ----------------------------------------------------------- */

typedef struct {
	const uint8_t *	val;		/* into the mapped nxsterms image */
	uint32_t	tot_off;	/* offset of the u64 BE total counter; 0 = dead id */
	uint16_t	len;
} hterm_t;

struct qprep;

/* one snapshot of the two index files: the four words nxs_index_changed() reads
 * (doc-shard refresh: every shard consumes exactly up to it) */
typedef struct {
	uint64_t	terms_len, dtmap_len;	/* data_len of nxsterms / nxsdtmap */
	uint64_t	hdr_docs, hdr_tokens;	/* nxsdtmap header counters */
} nxs_snap_t;

/* a doc shard's share of one refresh, walked and validated on the host (nxs_index.c) */
typedef struct nxs_delta nxs_delta_t;

/* one batch between nxs_index_search_batch_begin and _end */
typedef struct nxs_pend {
	bool		active;
	bool		on_device;	/* queued through nxsgpu_batch_begin */
	bool		want_total;	/* params "total": count every query's matches */
	bool		want_explain;	/* params "explain": per-token contributions of every result (explain_batch) */
	struct qprep *	xprep;		/* [n] or NULL: "explain" on a query-sharded batch whose every response this rank
					 * materialises -- the plans of the OTHER ranks' slices (this rank's are prep) */
	size_t		n;		/* queries of the whole batch */
	size_t		lo, hi;		/* this rank's slice */
	uint32_t	cap;		/* record slots per rank */
	int		rank, world;
	uint64_t	limit;
	int		algo;
	struct qprep *	prep;		/* [hi - lo] */
	uint64_t	seq;
	/*
	 * The batch's misses are being resolved on the device (nxsgpu_fuzzy_begin) and _begin has returned:
	 * the rest of its front half -- winners into the token lists, compile, queueing on the device -- is
	 * done by the next _begin (after ITS parse) or by this batch's _end, whichever comes first
	 * (nxs_batch.c: late_finish).  NULL otherwise.
	 */
	struct late_half *late;
	/*
	 * Collected early: the index files changed while this batch was in flight and
	 * a later _begin had to finish it to re-sync (search.c:309-312).  Its
	 * responses wait here for the caller's _end.
	 */
	bool		stashed;
	nxs_resp_t **	st_resps;	/* [n] */
	nxs_err_t *	st_errs;	/* [n] */
	int		st_ret;
	nxs_err_t	st_errcode;
	char *		st_errmsg;
} nxs_pend_t;

struct nxs_index {
	nxs_t *		nxs;
	char *		name;
	int		algo;		/* NXSGPU_BM25 / NXSGPU_TF_IDF */
	bool		lowercase;	/* open_files(): the pipeline is { normalizer } */
	struct nxs_filters *filters;	/* filter pipeline of query tokens, or NULL */

	uint8_t *	tmap;	size_t tmap_len;
	uint8_t *	dmap;	size_t dmap_len;

	/* term dictionary: ids 1..last_id (file order, terms.c:404) */
	hterm_t *	terms;
	uint32_t	last_id;
	uint32_t	term_count;
	uint32_t *	thash;		/* open addressing: term ids */
	size_t		thash_cap;

	uint64_t	n_docs;
	nxsgpu_index_t *dev;
	int		device;		/* HIP device of the index (NXS_GPU_DEVICE at open) */

	/* query sharding (nxs_index_shard) and the batches in flight */
	nxsgpu_comm_t *	comm;
	struct nxs_pend	pend[NXSGPU_INFLIGHT];
	/* tests: the n-th next _begin / exact fix-up of this index fails (0: off) */
	unsigned	test_fail_begin, test_fail_fixup, test_fail_fixup_recv, test_fail_late;
	bool		resync_pending;	/* sharded: a rank's block flags said its files moved */
	struct plan_cache *pcache;	/* query string -> compiled plan (nxs_plan.c: plan_batch) */
	uint64_t	pend_seq;
	/* host-side phase times of the batches, seconds (nxs_index_host_profile) */
	double		hp_plan, hp_queue, hp_wait, hp_resps, hp_begin, hp_end, hp_fzwait, hp_front, hp_fzlaunch, hp_back;
	uint64_t	hp_batches, hp_inexact;
	/* doc-sharded mode (N4): this index is shard `shard` of `n_shards` (0 = whole) */
	unsigned	shard, n_shards;
	int		want_device;	/* explicit device + 1, or 0: NXS_GPU_DEVICE / device 0 */
	bool		global_df_set;
	/* a doc-shard refresh failed after some device state changed: searches are refused
	 * until the next refresh rebuilds the collection (nxs_docshard_refresh) */
	bool		ds_inconsistent;
	unsigned	test_fail_dsref;	/* tests: the n-th next device step of a shard refresh fails */
	const nxs_snap_t *pin;		/* load / rebuild up to this snapshot (NULL: the file headers) */
	bool		shard_local;	/* nxs_index_shard_local: responses of the own slice only */
	int8_t		late_mode;	/* 0 not read yet, 1 a batch's fuzzy pass is left running (late_finish), 2 NXS_LATE_FUZZY=0:
					 * _begin waits for it itself */
	/* tests: play one rank of emu_world (nxs_test_shard_emulate) */
	int		emu_rank, emu_world;
	uint8_t *	emu_block;
	size_t		emu_block_len;

	/* what idx_terms_sync / idx_dtmap_sync have consumed (bytes of the data areas)
	 * and the header counters the device statistics were computed from */
	char *		terms_path;
	char *		dtmap_path;
	uint64_t	terms_consumed, dt_consumed;
	uint64_t	hdr_docs_seen, hdr_tokens_seen;
	size_t		terms_cap;
	/* persistent doc table, ordinal order (= ascending doc id) */
	uint64_t *	h_doc_ids;
	uint64_t *	h_blk_off;	/* block offset in the nxsdtmap image */
	uint32_t *	h_npairs;
	uint8_t *	h_alive;
	uint64_t	n_ord, cap_ord;
	/* host BK-tree (terms inserted up to bk_upto) behind the device image */
	struct nxs_bktree *bktree;
	uint32_t	bk_upto;
	bool		bk_flags_stale;
	/* the "total > 0" flag of every node of the image the device holds, BFS order (bk_flags_keep) */
	uint8_t *	bk_flags;
	uint32_t	bk_flags_n;
	uint64_t	n_incremental, n_rebuilds;
};

/* nxs_index.c */
int	nxs_index_load(nxs_index_t *, const char *terms_path, const char *dtmap_path);
void	nxs_index_unload(nxs_index_t *);
int	nxs_index_refresh(nxs_index_t *);
bool	nxs_index_changed(const nxs_index_t *);
int	nxs_index_bk_sync(nxs_index_t *);
void	nxs_index_refresh_stats(const nxs_index_t *, uint64_t out[2]);
/* doc-shard refresh (N4): the pieces of nxs_index_refresh, driven per collection by nxs_docshard.c */
void	nxs_index_snapshot(const nxs_index_t *, nxs_snap_t *);
int	nxs_shard_walk(nxs_index_t *, const nxs_snap_t *, uint64_t max_id, bool take_new, nxs_delta_t **);
int	nxs_shard_merge(nxs_index_t *, nxs_delta_t *);
void	nxs_delta_abort(nxs_index_t *, nxs_delta_t *);
int	nxs_shard_rebuild(nxs_index_t *, const nxs_snap_t *);
uint32_t nxs_term_lookup(const nxs_index_t *, const uint8_t *val, size_t len);
bool	nxs_index_doc_live(const nxs_index_t *, uint64_t doc_id) __attribute__((visibility("hidden")));

/* flattened BK-tree built on the host (exported for the CPU-side tests) */
typedef struct {
	nxsgpu_bknode_t *nodes;
	uint32_t	n;
	uint32_t	depth;
	uint8_t *	bytes;
	uint64_t	bytes_len;
} nxs_bkimage_t;

typedef struct nxs_bktree nxs_bktree_t;

nxs_bktree_t *nxs_bktree_create(void);
void	nxs_bktree_destroy(nxs_bktree_t *);
int	nxs_bktree_insert(nxs_bktree_t *, const hterm_t *terms, uint32_t from_id, uint32_t last_id);
int	nxs_bk_flatten(const nxs_bktree_t *, const hterm_t *terms, const uint8_t *tmap,
	    nxs_bkimage_t *out);
int	nxs_bk_build(const hterm_t *terms, uint32_t last_id, const uint8_t *tmap,
	    nxs_bkimage_t *out);
void	nxs_bk_free(nxs_bkimage_t *);

/* ---- filter pipeline of query tokens (nxs_filters.c) ------------------------ */

typedef struct nxs_filters nxs_filters_t;

nxs_filters_t *nxs_filters_create(const char *basedir, const char *const *names, size_t n,
	    const char *lang, const char **err);
void	nxs_filters_destroy(nxs_filters_t *);
int	nxs_filters_run(nxs_filters_t *, char **val, size_t *len);
/* ... on the stages of the pipeline that are in `stages` only (a query prefix: the normalizer alone) */
#define	NXS_FSTAGE_NORMALIZER	(1u << 1)
#define	NXS_FSTAGE_STOPWORDS	(1u << 2)
#define	NXS_FSTAGE_STEMMER	(1u << 3)
int	nxs_filters_run_stages(nxs_filters_t *, unsigned stages, char **val, size_t *len);
/* the index's pipeline on `stages`, or the ASCII lowercase when the index has `lowercase` only
 * (hidden: the library's export table is the headers' declarations, not this one) */
int	nxs_index_filter(const nxs_index_t *, unsigned stages, char **val, size_t *len)
	    __attribute__((visibility("hidden")));
/* the English Snowball stemmer (Porter2) on a UTF-8 token, in place -> new length (nxs_stem_en.c) */
size_t	nxs_stem_en(char *w, size_t len);

/* ---- query ----------------------------------------------------------- */

typedef enum {
	QTK_EOF = 0, QTK_AND, QTK_OR, QTK_NOT, QTK_BR_OPEN, QTK_BR_CLOSE,
	QTK_FF_STRING, QTK_QUOTED_STRING,
} qtoken_t;

/* postfix item: a leaf string or an operator */
typedef struct {
	uint8_t		op;	/* 0 = leaf, else NXSGPU_OP_AND/OR/ANDNOT */
	char *		str;	/* leaf value (owned) */
	int		token;	/* leaf: index into the token list, -1 = none */
} qitem_t;

typedef struct {
	qitem_t *	items;
	size_t		n;
	bool		error;
	char *		errmsg;
	/* one block for everything the front half of a query allocates */
	char *		arena;
	size_t		arena_used, arena_cap;
} qparse_t;

int	nxs_query_lex(const char *query, int *kinds, size_t cap);
void	nxs_query_parse(const char *query, qparse_t *out);
void	nxs_query_free(qparse_t *);
char *	nxs_query_repr(const qparse_t *);

typedef struct {
	char *		value;
	size_t		len;
	uint32_t	term_id;	/* 0 = unresolved */
} qtok_t;

/*
 * A prefix leaf (`term*` under "prefixmatch"): the normalised prefix, and -- once the batch's prefixes have
 * been resolved (nxsgpu_complete) -- its expansions: the first min(prefix_limit, matches) eligible terms in
 * the order df descending, term id ascending.  nxs_query_splice puts them in the leaf's place.
 */
#define	NXS_PREFIX_MAX		32	/* "prefix_limit" / "wildcard_terms" at most */
/*
 * A wildcard leaf (a `*` or `?` and at least one other byte, under "wildcardmatch") is recorded the same way:
 * `val` is the normalised pattern (nxs_wild_normalize), the expansions come from nxsgpu_wildcard and number
 * min(wildcard_terms, matches).
 */
/*
 * A doc leaf (nxs_index_similar: a program of this one leaf, nxs_query_prepare_doc): `val` carries the source
 * doc's id in decimal, the expansions come from nxsgpu_doc_terms -- the first min(similar_terms, matches)
 * eligible terms of the doc's term vector at mindf = similar_mindf.  Never plan-cached, never fuzzy-matched.
 */
enum { QPFX_PREFIX = 0, QPFX_WILD = 1, QPFX_DOC = 2 };
typedef struct {
	size_t		item;		/* the leaf: index into parse.items */
	int		kind;		/* QPFX_* */
	char *		val;		/* malloc'd, NUL-terminated */
	size_t		len;
	uint32_t	n;		/* expansions */
	uint32_t	ids[NXS_PREFIX_MAX];
	const uint8_t *	tval[NXS_PREFIX_MAX];	/* their bytes (the dictionary's) */
	uint16_t	tlen[NXS_PREFIX_MAX];
} qpfx_t;

typedef struct qprep {
	qparse_t	parse;
	qtok_t *	tokens;		/* token-list order (query.c:89-95) */
	size_t		n_tokens;
	nxs_err_t	errcode;	/* set when the query cannot run */
	char *		errmsg;
	bool		empty;		/* no live tokens: empty result */
	bool		wide;		/* does not fit nxsgpu_query_t: wplan is its plan */
	bool		cached;		/* the plan came from the index's plan cache: nothing was parsed */
	bool		compiled;	/* plan_batch: compiled in the first pass already (no token waits for the fuzzy search) */
	nxsgpu_query_t	plan;
	nxsgpu_wide_query_t wplan;	/* arrays owned by this object */
	char **		heap_vals;	/* token values a filter grew beyond the arena's reserve */
	size_t		n_heap_vals;
	qpfx_t *	pfx;		/* prefix leaves, in the order they were met (right to left) */
	size_t		n_pfx;
	bool		has_prefix;	/* some leaf was read as a prefix: the plan depends on prefix_limit and the df */
	void *		splice;		/* nxs_query_splice: the items, tokens and strings that replaced the arena's */
} qprep_t;

void	nxs_query_prepare(const nxs_index_t *, const char *query, qprep_t *out);
/* the query of nxs_index_similar: one doc leaf (QPFX_DOC), no token */
void	nxs_query_prepare_doc(nxs_doc_id_t doc, qprep_t *out);
/* the same; prefixmatch: a leaf from a free-form string that ends in `*` (and is longer) is a prefix leaf --
 * kept out of the token list, recorded in out->pfx */
void	nxs_query_prepare_px(const nxs_index_t *, const char *query, bool prefixmatch, qprep_t *out);
/* the same with both flags; wildcardmatch: a leaf from a free-form string that holds a `*` or `?` and at least
 * one other byte is a wildcard leaf -- unless prefixmatch is set too and it is a literal followed by a single
 * trailing `*`, which stays the prefix leaf it is.  A pattern that normalises to more than NXS_WILD_MAXLEN
 * bytes fails its query (NXS_ERR_INVALID "wildcard pattern too long") */
void	nxs_query_prepare_wc(const nxs_index_t *, const char *query, bool prefixmatch, bool wildcardmatch, qprep_t *out);
/*
 * A wildcard pattern as the matcher takes it: cut at its metacharacters, every literal piece through the
 * normalizer / lowercase stage only (the rule of a prefix: a fragment is not a word), put back together, runs
 * of `*` collapsed to one.  idx NULL: no filters.  1 = *out (malloc'd, NUL-terminated) / *out_len; 0 = no
 * literal byte is left (not served); -1 = the filters failed, -2 = out of memory, -3 = longer than
 * NXS_WILD_MAXLEN.  *literals (may be NULL) = its bytes that are no metacharacter.
 */
int	nxs_wild_normalize(const nxs_index_t *, const char *str, size_t len, char **out, size_t *out_len, size_t *literals)
	    __attribute__((visibility("hidden")));
/* every prefix leaf becomes (e1 OR e2 OR ... OR em), the token list what the rewritten query's would be;
 * m = 0: the leaf stays the empty set.  0 / -1 (out of memory) */
int	nxs_query_splice(qprep_t *);
int	nxs_query_compile(qprep_t *);	/* after term ids are final */
void	nxs_query_release(qprep_t *);
void	nxs_query_release_scratch(qprep_t *);	/* parse + token list; keeps errors and plans */

#endif
