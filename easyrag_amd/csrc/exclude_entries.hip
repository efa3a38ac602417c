// The exclude entries of the C ABI (include/easyrag_hip.h): erh_dense_topk_excl and erh_bm25_topk_excl, exact top k of what a query may see
// except a per-query id list (DESIGN K12; kernel: exclude.hip).  Each entry is: validate -> work space -> the exclusion CSR up, one upload ->
// the route's sets pipeline (dense_sets_run / bm25_sets_run, api.hip) at depth kk = k + the call's longest exclusion list, into buffers of
// the handle -> the drop kernel into the caller's rows.  No scan kernel knows about exclusions.  No CPU compute path lives here.
#include "../../include/easyrag_hip.h"
#include "handle.h"

// The exclusion lists of a call: a monotone CSR from 0, every list strictly ascending inside [0, N).  *e_max: the longest list.
static int check_excl_lists(erh_handle *h, const char *who, const int32_t *excl_ptr, const int32_t *excl_ids, int B, int64_t N, int *e_max) {
    const std::string w(who);
    *e_max = 0;
    if (excl_ptr[0] != 0) return h->fail(ERH_ERR_INVALID, (w + ": excl_ptr[0] != 0").c_str());
    for (int b = 0; b < B; ++b)
        if (excl_ptr[b + 1] < excl_ptr[b]) return h->fail(ERH_ERR_INVALID, (w + ": excl_ptr decreases").c_str());
    if (excl_ptr[B] > 0 && !excl_ids) return h->fail(ERH_ERR_INVALID, (w + ": null excl_ids").c_str());
    for (int b = 0; b < B; ++b) {
        for (int32_t i = excl_ptr[b]; i < excl_ptr[b + 1]; ++i) {
            const int32_t r = excl_ids[i];
            if (r < 0 || (int64_t)r >= N) return h->fail(ERH_ERR_INVALID, (w + ": excluded id outside [0, N)").c_str());
            if (i > excl_ptr[b] && r <= excl_ids[i - 1])
                return h->fail(ERH_ERR_INVALID, (w + ": the ids of an exclusion list must be strictly ascending").c_str());
        }
        *e_max = std::max(*e_max, excl_ptr[b + 1] - excl_ptr[b]);
    }
    return ERH_OK;
}

// The sub-query batch behind the class sets of a call, or -- both pointers null -- one sub-query without a class per query.
static int excl_sub_queries(erh_handle *h, const char *who, const int32_t *set_ptr, const int16_t *set_cls, int B, int64_t n_docs,
                            std::vector<int32_t> &sub_ptr, std::vector<int32_t> &src, std::vector<int16_t> &cls) {
    if (!set_ptr) {
        if (set_cls) return h->fail(ERH_ERR_INVALID, (std::string(who) + ": set_cls without set_ptr").c_str());
        sub_ptr.resize((size_t)B + 1);
        for (int b = 0; b <= B; ++b) sub_ptr[(size_t)b] = b;
        src.assign(sub_ptr.begin(), sub_ptr.begin() + B);
        cls.assign((size_t)B, (int16_t)-1);
        return ERH_OK;
    }
    const int rc = check_class_sets(h, who, set_ptr, set_cls, B, n_docs);
    if (rc == ERH_OK) expand_class_sets(h, set_ptr, set_cls, B, sub_ptr, src, cls);
    return rc;
}

static int excl_depth(erh_handle *h, const char *who, int k, int e_max, int limit, int *kk) {
    *kk = k + e_max;
    if (*kk <= limit) return ERH_OK;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: kk = k + longest exclusion list = %d + %d = %d > %d", who, k, e_max, *kk, limit);
    return h->fail(ERH_ERR_UNSUPPORTED, msg);
}

// Work space of a call, before anything is enqueued
static int excl_ensure(erh_handle *h, const char *who, erh_handle::ExclBufs &X, int B, int kk, HostOut &out) {
    hipError_t e = X.ids.ensure((size_t)B * kk * 4);
    if (e == hipSuccess) e = X.sc.ensure((size_t)B * kk * 8);
    if (e == hipSuccess) e = X.len.ensure((size_t)B * 4);
    if (e == hipSuccess) e = out.ensure();
    if (e == hipSuccess) return ERH_OK;
    (void)hipGetLastError();
    return h->fail(ERH_ERR_NOMEM, (std::string(who) + ": work space").c_str(), e);
}

static int excl_drop(erh_handle *h, int prof_class, const erh_handle::ExclBufs &X, int B, int k, int kk, HostOut &out, hipStream_t st) {
    const int32_t *d_ptr = X.tab.as<int32_t>();
    { ProfScope ps(h, st, prof_class, (double)B * kk * 12, 0);
      HIPCHK(h, erh::launch_topk_drop(X.ids.as<int32_t>(), X.sc.as<double>(), X.len.as<int32_t>(), kk, d_ptr, d_ptr + B + 1, B, k, out.d_ids,
                                      out.d_sc, out.d_len, st)); }
    h->stats.excl_drop_launches += 1;
    return out.finish(st);
}

extern "C" {

// The dense entry.  The inner batch is checked INSIDE the call (dense_sets_check: one stream synchronisation, further exhaustive rounds and
// the merge again where a sub-query was flagged) -- the drop kernel must read final lists --, so the contract is the rows entries': no
// erh_dense_check, host outputs final on return, device outputs after erh_sync.  The inner batch uses the scan route's work space (Q16,
// flags, cand, s_*, r_*): while an earlier device-output call waits for its check the entry refuses (ERH_ERR_STATE) instead of overwriting it.
int erh_dense_topk_excl(erh_handle *h, const void *q, int q_dtype, int q_is_device, int normalize_q, int B, int k,
                        const int32_t *set_ptr, const int16_t *set_cls, const int32_t *excl_ptr, const int32_t *excl_ids, int mode,
                        int32_t *out_ids, double *out_scores, int32_t *out_len, int out_is_device, void *stream) {
    if (!h) return ERH_ERR_INVALID;
    const char *who = "erh_dense_topk_excl";
    // (the depth limit is on kk, below: k itself is only checked for k < 1 here)
    int rc = check_dense_args(h, who, q, out_ids && out_scores && out_len && excl_ptr, B, std::min(k, 768), q_dtype, -1);
    if (rc != ERH_OK) return rc;
    if (mode != ERH_DENSE_EXACT && mode != ERH_DENSE_FAST) return h->fail(ERH_ERR_INVALID, "erh_dense_topk_excl: mode");
    std::vector<int32_t> sub_ptr, src;
    std::vector<int16_t> cls;
    rc = excl_sub_queries(h, who, set_ptr, set_cls, B, h->N, sub_ptr, src, cls);
    if (rc != ERH_OK) return rc;
    int e_max = 0, kk = 0;
    rc = check_excl_lists(h, who, excl_ptr, excl_ids, B, h->N, &e_max);
    if (rc == ERH_OK) rc = excl_depth(h, who, k, e_max, 768, &kk);
    if (rc != ERH_OK) return rc;
    if (h->check_pending)
        return h->fail(ERH_ERR_STATE, "erh_dense_topk_excl: an earlier device-output dense call still waits for erh_dense_check");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    HostOut out(h, out_ids, out_scores, out_len, out_is_device, B, k);
    rc = excl_ensure(h, who, h->xd, B, kk, out);
    if (rc != ERH_OK) return rc;
    TableBuilder tab;                                  // (read by the time dense_sets_run's synchronisation returns)
    tab.add(excl_ptr, (size_t)B + 1);
    tab.add(excl_ids, (size_t)excl_ptr[B]);
    HIPCHK(h, tab.upload(h->xd.tab, st));
    const void *qd = nullptr;
    if (!src.empty()) {
        rc = stage_query_block(h, q, q_dtype, q_is_device, B, st, &qd);
        if (rc != ERH_OK) return rc;
    }
    rc = dense_sets_run(h, qd, q_dtype, normalize_q, B, kk, sub_ptr, src, cls, mode, h->xd.ids.as<int32_t>(), h->xd.sc.as<double>(),
                        h->xd.len.as<int32_t>(), st);
    if (rc == ERH_OK) rc = dense_sets_check(h, st);
    h->forget_dense_call();                            // nothing of it is left for a later erh_dense_check; the diag words stay
    if (rc != ERH_OK) return rc;
    h->stats.dense_excl_calls += 1;
    return excl_drop(h, ERH_K_DENSE_SELECT, h->xd, B, k, kk, out, st);
}

// The sparse entry.  Its inner batch shares the scan's work space (qpack, part_*, bs_*): ordered with the handle's other scan calls like two
// erh_bm25_topk calls.  No flag words.
int erh_bm25_topk_excl(erh_handle *h, const int32_t *q_indptr, const int32_t *q_tok, int B, int k, const int32_t *set_ptr,
                       const int16_t *set_cls, const int32_t *excl_ptr, const int32_t *excl_ids, int32_t *out_ids, double *out_scores,
                       int32_t *out_len, int out_is_device, void *stream) {
    if (!h) return ERH_ERR_INVALID;
    const char *who = "erh_bm25_topk_excl";
    const Bm25State &S = h->bm[h->cur];
    if (S.variant < 0) return h->fail(ERH_ERR_STATE, "erh_bm25_topk_excl before erh_set_bm25_*");
    if (!q_indptr || !excl_ptr || !out_ids || !out_scores || !out_len || B <= 0)
        return h->fail(ERH_ERR_INVALID, "erh_bm25_topk_excl: null pointer or non-positive B");
    if (k < 1) return h->fail(ERH_ERR_UNSUPPORTED, "erh_bm25_topk_excl: k < 1");
    int rc = check_bm25_queries(h, who, q_indptr, q_tok, B, S.V);
    if (rc != ERH_OK) return rc;
    std::vector<int32_t> sub_ptr, src;
    std::vector<int16_t> cls;
    rc = excl_sub_queries(h, who, set_ptr, set_cls, B, S.Nb, sub_ptr, src, cls);
    if (rc != ERH_OK) return rc;
    int e_max = 0, kk = 0;
    rc = check_excl_lists(h, who, excl_ptr, excl_ids, B, S.Nb, &e_max);
    if (rc == ERH_OK) rc = excl_depth(h, who, k, e_max, 1024, &kk);
    if (rc != ERH_OK) return rc;
    if (!bm25_sets_tokens_fit(q_indptr, src))
        return h->fail(ERH_ERR_UNSUPPORTED, "erh_bm25_topk_excl: more than 2^31 query tokens in one chunk of sub-queries");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    HostOut out(h, out_ids, out_scores, out_len, out_is_device, B, k);
    rc = excl_ensure(h, who, h->xb, B, kk, out);
    if (rc != ERH_OK) return rc;
    TableBuilder tab;                                  // (read by the time bm25_sets_run's first synchronisation returns)
    tab.add(excl_ptr, (size_t)B + 1);
    tab.add(excl_ids, (size_t)excl_ptr[B]);
    HIPCHK(h, tab.upload(h->xb.tab, st));
    rc = bm25_sets_run(h, who, q_indptr, q_tok, B, kk, sub_ptr, src, cls, h->xb.ids.as<int32_t>(), h->xb.sc.as<double>(),
                       h->xb.len.as<int32_t>(), st);
    if (rc != ERH_OK) return rc;
    h->stats.bm25_excl_calls += 1;
    return excl_drop(h, ERH_K_BM25_MERGE, h->xb, B, k, kk, out, st);
}

}  // extern "C"
