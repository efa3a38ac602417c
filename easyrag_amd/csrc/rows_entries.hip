// The rows entries of the C ABI (include/easyrag_hip.h): erh_dense_topk_rows and erh_bm25_topk_rows, exact top k over explicit per-query row
// lists, and the scan route of their long lists (DESIGN K11; kernels: dense_rows.hip, bm25_rows.hip, rows_classes.hip).  Each entry is ONE
// pass: validate -> candidate lists and the rule's first answer -> work space -> row ids up -> (candidates: classify, the rule's second
// answer) -> shapes and small tables, one upload -> the scan batch -> the row-by-row shapes.  What they share with the sets entries
// (api.hip) is declared in handle.h.  No CPU compute path lives here.
#include "../../include/easyrag_hip.h"
#include "handle.h"

// The lists of a rows call: a monotone CSR from 0, every list strictly ascending inside [0, N), and list_of inside [-1, n_lists).
// *total: the entries of all lists.
static int check_row_lists(erh_handle *h, const char *who, int n_lists, const int64_t *list_ptr, const int32_t *list_rows, const int32_t *list_of,
                           int B, int64_t N, int64_t *total) {
    const std::string w(who);
    *total = 0;
    if (n_lists < 0 || (n_lists > 0 && !list_ptr)) return h->fail(ERH_ERR_INVALID, (w + ": negative n_lists or null list_ptr").c_str());
    if (n_lists > 0) {
        if (list_ptr[0] != 0) return h->fail(ERH_ERR_INVALID, (w + ": list_ptr[0] != 0").c_str());
        for (int l = 0; l < n_lists; ++l)
            if (list_ptr[l + 1] < list_ptr[l]) return h->fail(ERH_ERR_INVALID, (w + ": list_ptr decreases").c_str());
        *total = list_ptr[n_lists];
        if (*total > 0 && !list_rows) return h->fail(ERH_ERR_INVALID, (w + ": null list_rows").c_str());
        for (int l = 0; l < n_lists; ++l)
            for (int64_t i = list_ptr[l]; i < list_ptr[l + 1]; ++i) {
                const int32_t r = list_rows[i];
                if (r < 0 || (int64_t)r >= N) return h->fail(ERH_ERR_INVALID, (w + ": row outside [0, N)").c_str());
                if (i > list_ptr[l] && r <= list_rows[i - 1]) return h->fail(ERH_ERR_INVALID, (w + ": rows of a list must be strictly ascending").c_str());
            }
    }
    for (int b = 0; b < B; ++b)
        if (list_of[b] < -1 || list_of[b] >= n_lists) return h->fail(ERH_ERR_INVALID, (w + ": list_of outside [-1, n_lists)").c_str());
    return ERH_OK;
}

// ---- the scan route (DESIGN K11; kernels: rows_classes.hip) -------------------------------------------------------------------------------
// The long lists of a rows call become a call-local class column; the call's queries on those lists run through the sets pipelines
// (dense_sets_run, bm25_sets_run) on that column, installed in place of the handle's own class state for the duration of the call.

// Which lists of a call may take the scan route: named by a query, at least min_rows rows and longer than the short shape -- at most
// kRowsClassLists of them (more: none, the call keeps the row-by-row shapes).  bit[l]: the list's signature bit, -1 = not routed.
struct RowsScanPlan {
    std::vector<int32_t> bit;
    std::vector<int64_t> routed;             // {first entry, length} per routed list: what rows_sig_kernel reads
    std::vector<int32_t> n_q;                // queries per list
    int n_routed = 0, n_queries = 0, max_cells = 0, slots = 0;
    int64_t max_len = 0;
    void clear() { bit.assign(bit.size(), -1); routed.clear(); n_routed = n_queries = 0; }
};
static void rows_scan_candidates(int opt, int64_t min_rows, int n_lists, const int64_t *list_ptr, const int32_t *list_of, int B, int64_t N,
                                 RowsScanPlan *P) {
    P->bit.assign((size_t)n_lists, -1);
    P->n_q.assign((size_t)n_lists, 0);
    if (opt == 0 || N > 2147483647LL) return;
    for (int b = 0; b < B; ++b) if (list_of[b] >= 0) P->n_q[(size_t)list_of[b]] += 1;
    std::vector<int> cand;
    for (int l = 0; l < n_lists; ++l) {
        const int64_t len = list_ptr[l + 1] - list_ptr[l];
        if (P->n_q[l] > 0 && len >= min_rows && len > erh::kDenseRowsShortMax) cand.push_back(l);
    }
    if (cand.empty() || cand.size() > (size_t)erh::kRowsClassLists) return;
    int64_t entries = 0;
    for (int l : cand) {
        const int64_t len = list_ptr[l + 1] - list_ptr[l];
        P->bit[l] = P->n_routed++;
        P->routed.push_back(list_ptr[l]); P->routed.push_back(len);
        P->n_queries += P->n_q[l];
        P->max_len = std::max(P->max_len, len);
        entries += len;
    }
    // cells are non-empty and distinct: no more than entries, nor than the non-zero signatures of n_routed bits; one more than the column
    // can number is enough to see that there are too many
    int64_t bound = std::min<int64_t>(entries, (int64_t)erh::kRowsClassMax + 1);
    if (P->n_routed < 16) bound = std::min<int64_t>(bound, ((int64_t)1 << P->n_routed) - 1);
    P->max_cells = (int)bound;
    P->slots = erh::rows_classes_slots(bound);
}

// Which shape answers each query of a call, given the plan as it finally stands: the scan route where the query's list is routed (no entry
// here), the short shape for a list of at most short_max rows, the long shape for the rest.
struct RowsSplit {
    std::vector<int32_t> q_short, q_long;
    RowsSplit(const RowsScanPlan &P, const int64_t *list_ptr, const int32_t *list_of, int B, int64_t short_max) {
        for (int b = 0; b < B; ++b) {
            const int l = list_of[b];
            if (l >= 0 && P.bit[(size_t)l] >= 0) continue;
            ((l < 0 ? 0 : list_ptr[l + 1] - list_ptr[l]) <= short_max ? q_short : q_long).push_back(b);
        }
    }
};

// The host step: cells (signatures) -> the class sets of the call's queries.  bit_of[b]: the signature bit of query b's list, -1 = the query
// is not on the scan route (no sub-query).  Query b's set is every cell whose signature has its bit, in cell order.  False: the call keeps
// the row-by-row shapes (more lists than signature bits, more cells than an int16 column numbers).  Needs no device.
static bool rows_class_sets(const uint64_t *sig, int n_cells, int n_routed, const int32_t *bit_of, int B, std::vector<int32_t> &sub_ptr,
                            std::vector<int32_t> &src, std::vector<int16_t> &cls) {
    sub_ptr.assign((size_t)B + 1, 0);
    src.clear(); cls.clear();
    if (n_routed < 0 || n_routed > erh::kRowsClassLists || n_cells < 0 || n_cells > erh::kRowsClassMax) return false;
    // cells of every bit once, then every query copies its bit's
    std::vector<std::vector<int16_t>> of_bit((size_t)n_routed);
    for (int c = 0; c < n_cells; ++c)
        for (int l = 0; l < n_routed; ++l)
            if ((sig[c] >> l) & 1ull) of_bit[(size_t)l].push_back((int16_t)c);
    for (int b = 0; b < B; ++b) {
        const int l = bit_of[b];
        if (l >= 0 && l < n_routed)
            for (int16_t c : of_bit[(size_t)l]) { src.push_back(b); cls.push_back(c); }
        sub_ptr[(size_t)b + 1] = (int32_t)src.size();
    }
    return true;
}

// Buffers of the scan route (before anything is enqueued).  RowsClasses::table starts with the routed-list pairs, kRowsRoutedBytes of them.
static constexpr size_t kRowsRoutedBytes = (size_t)erh::kRowsClassLists * 2 * 8;
static hipError_t rows_classes_ensure(erh_handle::RowsClasses &rc, const RowsScanPlan &P, int64_t N) {
    hipError_t e = rc.sig.ensure((size_t)N * 8);
    if (e == hipSuccess) e = rc.cls.ensure((size_t)N * 2);
    if (e == hipSuccess) e = rc.table.ensure(kRowsRoutedBytes + erh::rows_classes_table_bytes(P.slots, P.max_cells));
    return e;
}

// The scan batch of a routed call: the class sets of its queries and the cells they name (read back into RowsClasses::cells_host).
struct RowsScanBatch {
    std::vector<int32_t> sub_ptr, src;
    std::vector<int16_t> cls;
    const erh::ErhRowsCell *cells = nullptr;
    int n_cells = 0;
};
// The candidates of plan P classified (rc.rows holds the call's row ids; the routed-list pairs go up here): signatures, cells, column, the
// cells read back (one copy; synchronises -- so the caller's row array has been read as well), the class sets, and the rule's second answer
// pays(batch), now that the cells are known.  1: the batch runs; 0: the call keeps the row-by-row shapes (too many cells, or the rule said
// no) and P is cleared -- nothing of the call's outputs has been written; < 0: an error.
template <typename Pays>
static int rows_scan_decide(erh_handle *h, erh_handle::RowsClasses &rc, RowsScanPlan &P, const int32_t *list_of, int B, int64_t N, int prof_class,
                            hipStream_t st, RowsScanBatch *R, Pays pays) {
    char *table = rc.table.as<char>() + kRowsRoutedBytes;
    HIPCHK(h, hipMemcpyAsync(rc.table.p, P.routed.data(), P.routed.size() * 8, hipMemcpyHostToDevice, st));
    { ProfScope ps(h, st, prof_class, (double)N * 26.0, 0);             // (each row: its word cleared, read twice, its class written)
      HIPCHK(h, erh::launch_rows_classes(rc.rows.as<int32_t>(), rc.table.as<int64_t>(), P.n_routed, P.max_len, N, P.slots, P.max_cells,
                                         rc.sig.as<unsigned long long>(), table, rc.cls.as<int16_t>(), st)); }
    const size_t bytes = 16 + (size_t)P.max_cells * sizeof(erh::ErhRowsCell);
    rc.cells_host.resize(bytes);
    HIPCHK(h, hipMemcpyAsync(rc.cells_host.data(), table, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    uint32_t hdr[4];
    memcpy(hdr, rc.cells_host.data(), 16);
    bool go = hdr[1] == 0u && hdr[0] <= (uint32_t)erh::kRowsClassMax && hdr[0] <= (uint32_t)P.max_cells;
    if (go) {
        R->cells = reinterpret_cast<const erh::ErhRowsCell *>(rc.cells_host.data() + 16);
        R->n_cells = (int)hdr[0];
        std::vector<uint64_t> sig((size_t)R->n_cells);
        for (int c = 0; c < R->n_cells; ++c) sig[(size_t)c] = R->cells[c].sig;
        std::vector<int32_t> bit_of((size_t)B, -1);
        for (int b = 0; b < B; ++b) if (list_of[b] >= 0) bit_of[(size_t)b] = P.bit[(size_t)list_of[b]];
        go = rows_class_sets(sig.data(), R->n_cells, P.n_routed, bit_of.data(), B, R->sub_ptr, R->src, R->cls) && pays(*R);
    }
    if (!go) P.clear();
    return go ? 1 : 0;
}

// What depends on the final shapes, held before any kernel that writes the call's outputs: the long shape's score spans and the small
// tables, which go up here.  Synchronises on every path: the table is pageable memory of the entry's scope, and so is the caller's row array.
static int rows_tables_up(erh_handle *h, const char *who, DevBuf &s64, int64_t need, TableBuilder &tab, DevBuf &buf, hipStream_t st) {
    hipError_t e = need > 0 ? s64.ensure((size_t)need * 8) : hipSuccess;
    if (e == hipSuccess) e = tab.upload(buf, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) return ERH_OK;
    (void)hipGetLastError();
    return h->fail(e == hipErrorOutOfMemory ? ERH_ERR_NOMEM : ERH_ERR_HIP, (std::string(who) + ": work space").c_str(), e);
}

// The class state of a handle -- everything it derives from erh_set_doc_meta's dir_id -- exchanged with a call-local column for the
// lifetime of this object: the column itself, its copy by stored position, the classes' row ranges and counts.  Dense dir blocks are off
// meanwhile (they would gather up to the whole matrix per call): the call scans through the filter column.  The destructor puts the
// handle's own state back, on every path; the call-local buffers return to `rc` for the next call.
struct CallClasses {
    erh_handle *h;
    erh_handle::RowsClasses &rc;
    bool on = false, has_dir = false, dir_pos_valid = false;
    int64_t Nmeta = 0;
    int dir_rng_n = 0, dense_dir_blocks = 0;
    std::vector<int32_t> lo, hi, cnt, order;
    std::vector<int64_t> off;
    erh_handle::DenseBlocks blocks;
    CallClasses(erh_handle *h_, erh_handle::RowsClasses &rc_) : h(h_), rc(rc_) {}
    CallClasses(const CallClasses &) = delete;
    CallClasses &operator=(const CallClasses &) = delete;
    void exchange() {
        std::swap(h->dir_id, rc.cls); std::swap(h->dir_pos, rc.pos); std::swap(h->dir_rng, rc.rng);
        std::swap(h->dir_lo_h, lo); std::swap(h->dir_hi_h, hi); std::swap(h->dir_cnt_h, cnt); std::swap(h->dir_order_h, order);
        std::swap(h->dir_off_h, off); std::swap(h->blocks, blocks);
    }
    // with_ranges: the cells' row ranges go up for bm25_dir_range (the copy is ordered in front of the call's scans on `st`)
    int enter(const erh::ErhRowsCell *cells, int n_cells, int64_t N, bool with_ranges, hipStream_t st) {
        if (with_ranges) {
            rc.rng_host.resize((size_t)n_cells * 2);
            for (int c = 0; c < n_cells; ++c) { rc.rng_host[2 * (size_t)c] = cells[c].lo; rc.rng_host[2 * (size_t)c + 1] = cells[c].hi; }
            HIPCHK(h, rc.rng.ensure((size_t)n_cells * 8));
            HIPCHK(h, hipMemcpyAsync(rc.rng.p, rc.rng_host.data(), (size_t)n_cells * 8, hipMemcpyHostToDevice, st));
            HIPCHK(h, hipStreamSynchronize(st));             // (rng_host is pageable and reused by the next routed call, whatever its stream;
                                                             //  8 bytes per cell, and the stream is idle: the tables were just uploaded)
        }
        has_dir = h->has_dir; dir_pos_valid = h->dir_pos_valid; Nmeta = h->Nmeta; dir_rng_n = h->dir_rng_n;
        dense_dir_blocks = h->opt_dense_dir_blocks;
        exchange();
        on = true;
        h->has_dir = true; h->dir_pos_valid = false; h->Nmeta = N; h->dir_rng_n = with_ranges ? n_cells : 0;
        h->opt_dense_dir_blocks = 0;
        h->dir_lo_h.resize((size_t)n_cells); h->dir_hi_h.resize((size_t)n_cells); h->dir_cnt_h.resize((size_t)n_cells);
        for (int c = 0; c < n_cells; ++c) { h->dir_lo_h[c] = cells[c].lo; h->dir_hi_h[c] = cells[c].hi; h->dir_cnt_h[c] = cells[c].cnt; }
        return ERH_OK;
    }
    ~CallClasses() {
        if (!on) return;
        exchange();
        h->has_dir = has_dir; h->dir_pos_valid = dir_pos_valid; h->Nmeta = Nmeta; h->dir_rng_n = dir_rng_n;
        h->opt_dense_dir_blocks = dense_dir_blocks;
    }
};

// ---- the work rule of either route, and the entries -------------------------------------------------------------------------------------------
static bool dense_rows_scan_pays(const erh_handle *h, const RowsScanPlan &P, int64_t n_sub, int64_t n_sub_small) {
    // the row-by-row work: every routed list is loaded once per group of kDenseRowsGroup queries; the scan's: N rows x the sub-queries'
    // columns, a scan narrower than the ridge counted as the ridge (HBM-bound).  One constant (gain) relates the two.  n_sub_small of the
    // n_sub sub-queries are on cells so small that the seed prefix holds fewer than k of their rows (dense_rows_cell_is_small): the
    // pipeline has no threshold to prune them with, and each costs dense_rows_scan_small_cell ordinary sub-queries.
    double today = 0;
    for (size_t l = 0; l < P.bit.size(); ++l)
        if (P.bit[l] >= 0) today += (double)((P.n_q[l] + erh::kDenseRowsGroup - 1) / erh::kDenseRowsGroup) * (double)P.routed[2 * (size_t)P.bit[l] + 1];
    const double cols = (double)(n_sub - n_sub_small) + (double)n_sub_small * (double)h->opt_dense_rows_scan_small_cell;
    const double scan = (double)h->N * std::max(cols, (double)h->opt_route_ridge);
    return today * (double)h->opt_dense_rows_scan_gain > scan;
}
static bool dense_rows_cell_is_small(const erh_handle *h, int64_t cell_rows, int k) {
    const int64_t n0 = std::min<int64_t>(h->opt_n0, h->N);               // the seed prefix is an even sample: cell_rows * n0 / N of them are the cell's
    return (double)cell_rows * (double)n0 < (double)k * (double)h->N;
}

static bool bm25_rows_scan_pays(const erh_handle *h, const RowsScanPlan &P, int64_t N, int64_t n_sub, int64_t n_cells) {
    // the row-by-row work: (query, listed row) pairs; the scan's: (sub-query, row) pairs, every cell counted as `floor` sub-queries more (what
    // the scan route costs before its first sub-query, and with every further class a batch is spread over).  One constant (gain) relates the two.
    double today = 0;
    for (size_t l = 0; l < P.bit.size(); ++l)
        if (P.bit[l] >= 0) today += (double)P.n_q[l] * (double)P.routed[2 * (size_t)P.bit[l] + 1];
    const double scan = (double)N * ((double)n_sub + (double)h->opt_bm25_rows_scan_floor * (double)n_cells);
    return today * (double)h->opt_bm25_rows_scan_gain > scan;
}

extern "C" {

// Explicit row lists (dense_rows.hip).  The call keeps to buffers of its own (rw_*, rwc) and touches neither the flag words nor the record of
// the last scan-route call: it has no threshold to verify, so nothing of it is left for erh_dense_check, and a device-output dense call that
// is still waiting for its check finds everything as it left it.  Queries are prepared by the same kernel as on every other route (the fp16
// values the scores are defined on).  Lists of at most kDenseRowsShortMax rows: one launch for all their queries; longer ones: score + select
// launches per chunk of queries whose score spans fit the work space -- chunks follow each other on the stream, which is what orders the reuse
// of the span buffer; the work-item tables of the whole call go up once, the row ids straight from the caller's array.
//   The scan route (DESIGN K11): the call's long lists that the work rule sends there (options dense_rows_scan, dense_rows_scan_min_rows) become
// a call-local class column (rows_classes.hip) and their queries one set-filtered batch of the scan pipeline (dense_sets_run) on that column,
// installed for the call by a CallClasses guard.  That batch is checked INSIDE the call (its flag words and exhaustive rounds read the
// column), so the entry's contract stands: no erh_dense_check, host outputs final on return, device outputs after erh_sync.  The merge
// writes every row of the batch (an empty list for the queries that are not on the route); the short and long shapes then overwrite theirs.
// While a device-output scan-route call waits for its check (check_pending) the scan route is off: it would clobber that call's work space.
//   One pass: the candidates are classified BEFORE the shapes are laid out.  When the classification gives up (too many cells) or the rule
// says no once the cells are known, the plan is cleared and the same pass lays every query out on the row-by-row shapes: the lists were
// validated once, the row ids went up once, and there is one table.
int erh_dense_topk_rows(erh_handle *h, const void *q, int q_dtype, int q_is_device, int normalize_q, int B, int k,
                        int n_lists, const int64_t *list_ptr, const int32_t *list_rows, const int32_t *list_of,
                        int32_t *out_ids, double *out_scores, int32_t *out_len, int out_is_device, void *stream) {
    if (!h) return ERH_ERR_INVALID;
    const char *who = "erh_dense_topk_rows";
    int rc = check_dense_args(h, who, q, out_ids && out_scores && out_len && list_of, B, k, q_dtype, -1);
    if (rc != ERH_OK) return rc;
    const int64_t N = h->N;
    const int d = h->d;
    int64_t total = 0;
    rc = check_row_lists(h, who, n_lists, list_ptr, list_rows, list_of, B, N, &total);
    if (rc != ERH_OK) return rc;
    auto len_of = [&](int b) -> int64_t { const int l = list_of[b]; return l < 0 ? 0 : list_ptr[l + 1] - list_ptr[l]; };
    // (decided from the list lengths alone, before any routing: the status of a call does not depend on the rule)
    for (int b = 0; b < B; ++b)
        if (len_of(b) > erh::kDenseRowsShortMax && erh::dense_rows_score_lds(d) > 128 * 1024)
            return h->fail(ERH_ERR_UNSUPPORTED, "erh_dense_topk_rows: d too large for lists longer than 2048 rows");
    RowsScanPlan SP;
    const int scan_opt = h->check_pending ? 0 : h->opt_dense_rows_scan;
    rows_scan_candidates(scan_opt, h->opt_dense_rows_scan_min_rows, n_lists, list_ptr, list_of, B, N, &SP);
    if (SP.n_routed && scan_opt == 1 && !dense_rows_scan_pays(h, SP, SP.n_queries, 0)) SP.clear();   // (a query is at least one sub-query)
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    // work space first: a call that cannot have it enqueues nothing (what depends on the final shapes: below, before any kernel that writes
    // the call's outputs)
    const size_t q_bytes = (size_t)B * d * (q_dtype == ERH_F16 ? 2 : 4);
    HostOut out(h, out_ids, out_scores, out_len, out_is_device, B, k);
    out.b_ids = &h->rw_ids; out.b_sc = &h->rw_sc; out.b_len = &h->rw_len;
    {
        hipError_t e = h->rwc.rows.ensure((size_t)std::max<int64_t>(total, 1) * 4);
        if (e == hipSuccess) e = h->rw_q16.ensure((size_t)B * d * 2);
        if (e == hipSuccess) e = h->rw_qn.ensure((size_t)B * 4);
        if (e == hipSuccess && !q_is_device) e = h->rw_q.ensure(q_bytes);
        if (e == hipSuccess && SP.n_routed) e = rows_classes_ensure(h->rwc, SP, N);
        if (e == hipSuccess) e = out.ensure();
        if (e != hipSuccess) { (void)hipGetLastError(); return h->fail(ERH_ERR_NOMEM, "erh_dense_topk_rows: work space", e); }
    }
    // (the caller's arrays are read by the time the next synchronisation returns: rows_scan_decide's, or the one behind the table upload)
    if (total > 0) HIPCHK(h, hipMemcpyAsync(h->rwc.rows.p, list_rows, (size_t)total * 4, hipMemcpyHostToDevice, st));
    if (!q_is_device) HIPCHK(h, hipMemcpyAsync(h->rw_q.p, q, q_bytes, hipMemcpyHostToDevice, st));
    const int32_t *d_rows = h->rwc.rows.as<int32_t>();
    RowsScanBatch R;
    if (SP.n_routed) {
        rc = rows_scan_decide(h, h->rwc, SP, list_of, B, N, ERH_K_DENSE_SELECT, st, &R, [&](const RowsScanBatch &R_) {
            if (scan_opt != 1) return true;
            int64_t n_small = 0;
            for (int16_t c : R_.cls) n_small += dense_rows_cell_is_small(h, R_.cells[c].cnt, k) ? 1 : 0;
            return dense_rows_scan_pays(h, SP, (int64_t)R_.src.size(), n_small);
        });
        if (rc < 0) return rc;
    }
    // the shapes of every query that is not on the scan route: the short one where the list fits the LDS sort, the long one for the rest,
    // grouped by list
    RowsSplit split(SP, list_ptr, list_of, B, erh::kDenseRowsShortMax);
    const std::vector<int32_t> &q_short = split.q_short;
    std::vector<int32_t> &q_long = split.q_long;
    std::stable_sort(q_long.begin(), q_long.end(), [&](int32_t a, int32_t b) { return list_of[a] < list_of[b]; });
    // chunks of long queries (whole list groups of <= kDenseRowsGroup where they fit) whose spans fit the work space; span offsets are relative
    // to the chunk
    const int64_t ws_doubles = std::max<int64_t>((h->opt_rows_ws_mb << 20) / 8, N);
    struct Chunk { int q0, q1; int64_t item0, item1, doubles; };
    std::vector<Chunk> chunks;
    std::vector<int64_t> span_off((size_t)B, 0);
    std::vector<erh::ErhRowsItem> items;
    {
        size_t i = 0;
        Chunk c{0, 0, 0, 0, 0};
        while (i < q_long.size()) {
            const int l = list_of[q_long[i]];
            const int64_t len = list_ptr[l + 1] - list_ptr[l];
            size_t j = i;
            while (j < q_long.size() && j - i < (size_t)erh::kDenseRowsGroup && list_of[q_long[j]] == l) ++j;
            int ng = (int)(j - i);
            if (c.doubles + len > ws_doubles && c.q1 > c.q0) {            // the chunk is full: it ends in front of this group
                c.item1 = (int64_t)items.size();
                chunks.push_back(c);
                c = Chunk{(int)i, (int)i, (int64_t)items.size(), 0, 0};
            }
            ng = (int)std::min<int64_t>(ng, std::max<int64_t>(1, (ws_doubles - c.doubles) / len));   // (len <= N <= ws_doubles: at least one)
            for (int g = 0; g < ng; ++g) { span_off[(size_t)q_long[i + g]] = c.doubles; c.doubles += len; }
            for (int64_t i0 = 0; i0 < len; i0 += erh::kDenseRowsSeg)
                items.push_back(erh::ErhRowsItem{list_ptr[l] + i0, (int32_t)std::min<int64_t>(erh::kDenseRowsSeg, len - i0), (int32_t)i0, (int32_t)i, ng});
            i += (size_t)ng;
            c.q1 = (int)i;
        }
        if (c.q1 > c.q0) { c.item1 = (int64_t)items.size(); chunks.push_back(c); }
    }
    int64_t need = 0;
    for (const Chunk &c : chunks) need = std::max(need, c.doubles);
    const int64_t zero = 0;
    TableBuilder tab;
    const auto s_ptr = tab.add(n_lists > 0 ? list_ptr : &zero, (size_t)n_lists + 1);
    const auto s_span = tab.add(span_off);
    const auto s_items = tab.add(items);
    const auto s_of = tab.add(list_of, (size_t)B);
    const auto s_short = tab.add(q_short);
    const auto s_long = tab.add(q_long);
    rc = rows_tables_up(h, who, h->rw_s64, need, tab, h->rw_tab, st);
    if (rc != ERH_OK) return rc;
    const int64_t *d_ptr = tab.at(s_ptr), *d_span = tab.at(s_span);
    const erh::ErhRowsItem *d_items = tab.at(s_items);
    const int32_t *d_of = tab.at(s_of), *d_short = tab.at(s_short), *d_long = tab.at(s_long);
    int32_t *d_ids = out.d_ids; double *d_sc = out.d_sc; int32_t *d_len = out.d_len;
    const _Float16 *X = h->X.as<_Float16>();
    const _Float16 *Q16 = h->rw_q16.as<_Float16>();
    if (SP.n_routed) {
        {
            CallClasses cc(h, h->rwc);
            rc = cc.enter(R.cells, R.n_cells, N, false, st);
            if (rc == ERH_OK) rc = dense_sets_run(h, q_is_device ? q : h->rw_q.p, q_dtype, normalize_q, B, k, R.sub_ptr, R.src, R.cls, ERH_DENSE_EXACT,
                                                  d_ids, d_sc, d_len, st);
            if (rc == ERH_OK) rc = dense_sets_check(h, st);   // (the flag words and the exhaustive rounds read the column: before it is restored)
            h->forget_dense_call();                           // nothing of it is left for a later erh_dense_check; the diag words stay
        }
        if (rc != ERH_OK) return rc;
        h->stats.dense_rows_scan_calls += 1;
        h->stats.dense_rows_scan_subqueries += (int64_t)R.src.size();
    }
    h->stats.dense_rows_calls += 1;
    if (!q_short.empty() || !chunks.empty()) {
        ProfScope ps(h, st, ERH_K_DENSE_SELECT, 0, 0);
        HIPCHK(h, erh::launch_prep_queries(q_is_device ? q : h->rw_q.p, q_dtype, normalize_q, B, B, d, h->rw_q16.as<_Float16>(), h->rw_qn.as<float>(),
                                           nullptr, nullptr, st));
    }
    if (!q_short.empty()) {
        int64_t n_rows = 0;
        for (int32_t b : q_short) n_rows += len_of(b);
        ProfScope ps(h, st, ERH_K_DENSE_SCAN, (double)n_rows * d * 2, 2.0 * (double)n_rows * d);
        HIPCHK(h, erh::launch_dense_rows_short(X, N, d, h->pos_mul, Q16, d_rows, d_ptr, d_of, d_short, (int)q_short.size(), k, d_ids, d_sc, d_len, st));
        h->stats.dense_rows_short += 1;
    }
    for (const Chunk &c : chunks) {
        { ProfScope ps(h, st, ERH_K_DENSE_SCAN, 0, (double)c.doubles * d * 2.0);
          HIPCHK(h, erh::launch_dense_rows_score(X, N, d, h->pos_mul, Q16, d_rows, d_items + c.item0, (int)(c.item1 - c.item0), d_long, d_span,
                                                 h->rw_s64.as<double>(), st)); }
        { ProfScope ps(h, st, ERH_K_DENSE_SELECT, (double)c.doubles * 8, 0);
          HIPCHK(h, erh::launch_dense_rows_select(h->rw_s64.as<double>(), d_span, d_rows, d_ptr, d_of, d_long + c.q0, c.q1 - c.q0, k, d_ids, d_sc,
                                                  d_len, st)); }
        h->stats.dense_rows_long += 1;
    }
    return out.finish(st);
}

// Explicit row lists on the sparse route (bm25_rows.hip; launches: pipeline_bm25.hip, bm25_rows_dev): the twin of erh_dense_topk_rows, one
// pass in the same order.  The call keeps to buffers of its own (bw_*, bwc) -- neither the query upload of erh_bm25_topk (qpack) nor the
// staging rows of any other entry are touched, so a device-output call enqueued in front of it on the stream keeps its results -- and sets
// no flag words.  Lists of at most kBm25RowsShortMax rows: one launch for all their queries; longer ones: score + select launches per chunk
// of queries whose score spans fit the work space.
//   The scan route (options bm25_rows_scan, bm25_rows_scan_min_rows) runs its batch through bm25_sets_run on the call-local column over the
// slot's documents.  That batch uses the scan's work space (qpack, part_*, bs_*): a routed call is ordered with the handle's other scan
// calls like two erh_bm25_topk calls are.  A call that the route does not take after all (too many cells, a chunk's tokens past 32 bits, the
// rule's second answer) carries on with every query on the row-by-row shapes.
int erh_bm25_topk_rows(erh_handle *h, const int32_t *q_indptr, const int32_t *q_tok, int B, int k,
                       int n_lists, const int64_t *list_ptr, const int32_t *list_rows, const int32_t *list_of,
                       int32_t *out_ids, double *out_scores, int32_t *out_len, int out_is_device, void *stream) {
    if (!h) return ERH_ERR_INVALID;
    const char *who = "erh_bm25_topk_rows";
    const Bm25State &S = h->bm[h->cur];
    if (S.variant < 0) return h->fail(ERH_ERR_STATE, "erh_bm25_topk_rows before erh_set_bm25_*");
    if (!q_indptr || !out_ids || !out_scores || !out_len || !list_of || B <= 0) return h->fail(ERH_ERR_INVALID, "erh_bm25_topk_rows: null pointer or non-positive B");
    if (k < 1 || k > 1024) return h->fail(ERH_ERR_UNSUPPORTED, "erh_bm25_topk_rows: k outside [1, 1024]");
    if (S.nnz >= ((int64_t)1 << 32)) return h->fail(ERH_ERR_UNSUPPORTED, "erh_bm25_topk_rows: more than 2^32 postings");
    int rc = check_bm25_queries(h, who, q_indptr, q_tok, B, S.V);
    if (rc != ERH_OK) return rc;
    const int nt = q_indptr[B];
    const int64_t N = S.Nb;
    int64_t total = 0;
    rc = check_row_lists(h, who, n_lists, list_ptr, list_rows, list_of, B, N, &total);
    if (rc != ERH_OK) return rc;
    auto len_of = [&](int b) -> int64_t { const int l = list_of[b]; return l < 0 ? 0 : list_ptr[l + 1] - list_ptr[l]; };
    auto ntok_of = [&](int b) -> int64_t { return q_indptr[b + 1] - q_indptr[b]; };
    RowsScanPlan SP;
    const int scan_opt = h->opt_bm25_rows_scan;
    rows_scan_candidates(scan_opt, h->opt_bm25_rows_scan_min_rows, n_lists, list_ptr, list_of, B, N, &SP);
    if (SP.n_routed && scan_opt == 1 && !bm25_rows_scan_pays(h, SP, N, SP.n_queries, 1)) SP.clear();   // (a query is at least one sub-query, the lists at least one cell)
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    // work space first: a call that cannot have it enqueues nothing (what depends on the final shapes: below, before any kernel that writes
    // the call's outputs)
    HostOut out(h, out_ids, out_scores, out_len, out_is_device, B, k);
    out.b_ids = &h->bw_ids; out.b_sc = &h->bw_sc; out.b_len = &h->bw_len;
    {
        hipError_t e = h->bwc.rows.ensure((size_t)std::max<int64_t>(total, 1) * 4);
        if (e == hipSuccess && SP.n_routed) e = rows_classes_ensure(h->bwc, SP, N);
        if (e == hipSuccess) e = out.ensure();
        if (e != hipSuccess) { (void)hipGetLastError(); return h->fail(ERH_ERR_NOMEM, "erh_bm25_topk_rows: work space", e); }
    }
    // (the caller's array is read by the time the next synchronisation returns: rows_scan_decide's, or the one behind the table upload)
    if (total > 0) HIPCHK(h, hipMemcpyAsync(h->bwc.rows.p, list_rows, (size_t)total * 4, hipMemcpyHostToDevice, st));
    RowsScanBatch R;
    if (SP.n_routed) {
        rc = rows_scan_decide(h, h->bwc, SP, list_of, B, N, ERH_K_BM25_MERGE, st, &R, [&](const RowsScanBatch &R_) {
            return bm25_sets_tokens_fit(q_indptr, R_.src) && (scan_opt != 1 || bm25_rows_scan_pays(h, SP, N, (int64_t)R_.src.size(), R_.n_cells));
        });
        if (rc < 0) return rc;
    }
    // shapes by list length; the long queries in chunks whose spans (offsets relative to the chunk) fit the work space, one work item per
    // (query, segment of kBm25RowsSeg rows)
    Bm25RowsPlan P;
    const RowsSplit split(SP, list_ptr, list_of, B, erh::kBm25RowsShortMax);
    const std::vector<int32_t> &q_short = split.q_short, &q_long = split.q_long;
    for (int32_t b : q_short) P.short_searches += len_of(b) * ntok_of(b);
    const int64_t ws_doubles = std::max<int64_t>((h->opt_bm25_rows_ws_mb << 20) / 8, N);
    std::vector<int64_t> span_off((size_t)B, 0);
    std::vector<erh::ErhBm25RowsItem> items;
    {
        Bm25RowsPlan::Chunk c{0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < q_long.size(); ++i) {
            const int32_t b = q_long[i];
            const int64_t len = len_of(b);                                // (len <= N <= ws_doubles: a chunk holds at least one query)
            if (c.doubles + len > ws_doubles && c.q1 > c.q0) {            // the chunk is full: it ends in front of this query
                c.item1 = (int64_t)items.size();
                P.chunks.push_back(c);
                c = Bm25RowsPlan::Chunk{(int)i, (int)i, (int64_t)items.size(), 0, 0, 0};
            }
            span_off[(size_t)b] = c.doubles;
            c.doubles += len;
            c.searches += len * ntok_of(b);
            for (int64_t i0 = 0; i0 < len; i0 += erh::kBm25RowsSeg)
                items.push_back(erh::ErhBm25RowsItem{b, (int32_t)i0, (int32_t)std::min<int64_t>(erh::kBm25RowsSeg, len - i0)});
            c.q1 = (int)i + 1;
        }
        if (c.q1 > c.q0) { c.item1 = (int64_t)items.size(); P.chunks.push_back(c); }
    }
    int64_t need = 0;
    for (const Bm25RowsPlan::Chunk &c : P.chunks) need = std::max(need, c.doubles);
    const int64_t zero = 0;
    TableBuilder tab;
    const auto s_ptr = tab.add(n_lists > 0 ? list_ptr : &zero, (size_t)n_lists + 1);
    const auto s_span = tab.add(span_off);
    const auto s_qptr = tab.add(q_indptr, (size_t)B + 1);
    const auto s_qtok = tab.add(q_tok, (size_t)nt);
    const auto s_of = tab.add(list_of, (size_t)B);
    const auto s_short = tab.add(q_short);
    const auto s_long = tab.add(q_long);
    const auto s_items = tab.add(items);
    rc = rows_tables_up(h, who, h->bw_s64, need, tab, h->bw_tab, st);
    if (rc != ERH_OK) return rc;
    P.d_ptr = tab.at(s_ptr); P.d_span = tab.at(s_span); P.d_qptr = tab.at(s_qptr); P.d_qtok = tab.at(s_qtok);
    P.d_rows = h->bwc.rows.as<int32_t>(); P.d_of = tab.at(s_of); P.d_short = tab.at(s_short); P.d_long = tab.at(s_long);
    P.d_items = tab.at(s_items);
    P.n_short = (int)q_short.size();
    if (SP.n_routed) {
        {
            CallClasses cc(h, h->bwc);
            rc = cc.enter(R.cells, R.n_cells, N, h->opt_bm25_dir_range != 0, st);
            if (rc == ERH_OK) rc = bm25_sets_run(h, who, q_indptr, q_tok, B, k, R.sub_ptr, R.src, R.cls, out.d_ids, out.d_sc, out.d_len, st);
        }
        if (rc != ERH_OK) return rc;
        h->stats.bm25_rows_scan_calls += 1;
        h->stats.bm25_rows_scan_subqueries += (int64_t)R.src.size();
    }
    h->stats.bm25_rows_calls += 1;
    rc = bm25_rows_dev(h, P, k, out.d_ids, out.d_sc, out.d_len, st);
    return rc == ERH_OK ? out.finish(st) : rc;
}

int erh_debug_rows_class_sets(int n_cells, const uint64_t *cell_sig, int n_routed, int B, const int32_t *bit_of, int32_t *sub_ptr,
                              int16_t *sub_cls, int sub_cap) {
    if (n_cells < 0 || (n_cells > 0 && !cell_sig) || B < 0 || (B > 0 && !bit_of) || !sub_ptr || sub_cap < 0 || (sub_cap > 0 && !sub_cls))
        return ERH_ERR_INVALID;
    std::vector<int32_t> ptr, src;
    std::vector<int16_t> cls;
    if (!rows_class_sets(cell_sig, n_cells, n_routed, bit_of, B, ptr, src, cls)) return ERH_ERR_UNSUPPORTED;
    if ((int64_t)cls.size() > (int64_t)sub_cap) return ERH_ERR_NOMEM;
    memcpy(sub_ptr, ptr.data(), ((size_t)B + 1) * 4);
    if (!cls.empty()) memcpy(sub_cls, cls.data(), cls.size() * 2);
    return ERH_OK;
}

}  // extern "C"
