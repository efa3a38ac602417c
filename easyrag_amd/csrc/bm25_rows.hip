// Sparse route over EXPLICIT ROW LISTS (erh_bm25_topk_rows, api.hip): query b ranks the rows of its list -- sorted, distinct document ids --
// by their BM25 score and nothing else.  What BM25Retriever.get_scores + .filter return when the keep mask is an id set: a dir of a few
// hundred chunks, an ACL's ids, a candidate list to re-score, and the sparse leg of a fused call held to one set.
//
// Why it is exact: EVERY listed row gets the library-order sum (include/easyrag_hip.h: the payloads of the query's terms in query order,
// repeats included, accumulated from 0 in the payload's type; an absent term adds + 0) -- the arithmetic of as_finish_query (bm25.hip) with
// the caller's list in place of the scan's survivors: one binary search per (row, query token) in the token's postings, narrowed by the skip
// table, the payloads laid out as an LDS matrix with an odd row length and summed in token order.  No scan, no fixed-point copy, no
// threshold: nothing is left to verify, and the sign of the payloads does not matter.  Rows with a score <= 0 are never returned
// (retrievers.py:195-196); the others are ranked by (score desc, row id asc), fp32 sums widened exactly.
//
// Two shapes, chosen per query by the length of its list:
//   short (<= kRowsCap = 2048 rows)  ONE launch, one workgroup per query: sums of all rows in LDS, the positive ones compacted and sorted
//                                    (bitonic over the next power of two), k entries out.
//   long  (any length up to N)       two launches per chunk of queries.  bm25_rows_score_kernel: one workgroup per (query, segment of 2048 rows)
//                                    writes the widened score of every row of the segment into the query's fp64 span.  bm25_rows_select_kernel:
//                                    one workgroup per query streams the span through a 2048-entry list kept under an exact (score, id)
//                                    threshold, appending only scores > 0.
// No atomics on results, no data-dependent scheduling between workgroups: deterministic.  Row ids ([0, N), strictly ascending) and term ids
// ([0, V)) are validated on the host before anything is enqueued, so no search can leave the postings.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRowsCap = erh::kBm25RowsShortMax;    // 2048: rows whose sums one workgroup holds = the select list
constexpr int kThreads = 256;                       // short and score kernels
constexpr int kSelectThreads = 1024;
constexpr int kTokChunk = 64;                       // query tokens per pass (as_finish_query: kAsTokChunk)
constexpr int kMBytes = 24 * 1024;                  // the (row, token) payload matrix: 3072 fp64 / 6144 fp32 entries
constexpr int kInFlight = 6;                        // searches in flight per thread (as_finish_query: R = 6)

struct TokTab {                                     // the query's token table of the current pass
    int32_t tok[kTokChunk];
    uint32_t first[kTokChunk];                      // first posting of the term
    uint32_t count[kTokChunk];                      // its postings
};

// cs[0 .. n) = the library-order sums, widened, of the rows lr[0 .. n) for the query tokens q_tok[qs .. qs + nq).  A sum is carried from one
// token pass to the next as a double: ST -> double -> ST is exact.  Uniform call; begins and ends with barriers.
template <typename ST>
__device__ __forceinline__ void bm_rows_sums(const erh::ErhBm25RowsIndex &ix, const int32_t *__restrict__ q_tok, int qs, int nq,
                                             const int32_t *__restrict__ lr, int n, double *cs, ST *M, TokTab *tt) {
    constexpr int kMCap = kMBytes / (int)sizeof(ST);
    constexpr int R = kInFlight;
    const int tid = threadIdx.x;
    const ST *__restrict__ payload = reinterpret_cast<const ST *>(ix.payload);
    const int32_t *__restrict__ doc_ids = ix.doc_ids;
    for (int i = tid; i < n; i += kThreads) cs[i] = 0.0;
    for (int c0 = 0; c0 < nq; c0 += kTokChunk) {
        const int nqc = nq - c0 < kTokChunk ? nq - c0 : kTokChunk;
        const int ld = nqc | 1;                                           // odd row length: conflict-free column walk
        __syncthreads();
        if (tid < nqc) {
            const int32_t tok = q_tok[qs + c0 + tid];
            const int64_t a = ix.indptr[tok];
            tt->tok[tid] = tok;
            tt->first[tid] = (uint32_t)a;
            tt->count[tid] = (uint32_t)(ix.indptr[tok + 1] - a);
        }
        __syncthreads();
        const int ec_max = kMCap / ld;                                    // >= 47 rows per pass
        for (int e0 = 0; e0 < n; e0 += ec_max) {
            const int ec = n - e0 < ec_max ? n - e0 : ec_max;
            const int items = ec * nqc;
            for (int w0 = tid; w0 < items; w0 += R * kThreads) {
                uint32_t lo[R], hi[R], hi0[R];
                int32_t doc[R];
                int mpos[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int w = w0 + r * kThreads;
                    lo[r] = hi[r] = hi0[r] = 0u;
                    doc[r] = 0;
                    mpos[r] = -1;
                    if (w < items) {
                        const int e = w / nqc, j = w - e * nqc;
                        doc[r] = lr[e0 + e];
                        if (ix.tile_off) {                                // the skip-table range that holds the document
                            const int32_t *to = ix.tile_off + (int64_t)tt->tok[j] * (ix.n_tab + 1) + (doc[r] >> ix.tab_shift);
                            lo[r] = tt->first[j] + (uint32_t)to[0];
                            hi[r] = hi0[r] = tt->first[j] + (uint32_t)to[1];
                        } else {                                          // the term's whole posting range
                            lo[r] = tt->first[j];
                            hi[r] = hi0[r] = tt->first[j] + tt->count[j];
                        }
                        mpos[r] = e * ld + j;
                    }
                }
                for (;;) {                                                // first posting with document >= doc, R at a time
                    bool act[R];
                    uint32_t mid[R];
                    int32_t dv[R];
                    bool any = false;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        act[r] = lo[r] < hi[r];
                        mid[r] = lo[r] + ((hi[r] - lo[r]) >> 1);
                        dv[r] = act[r] ? doc_ids[mid[r]] : 0;
                        any |= act[r];
                    }
                    if (!any) break;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (act[r]) { if (dv[r] < doc[r]) lo[r] = mid[r] + 1u; else hi[r] = mid[r]; }
                    }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (mpos[r] >= 0) {
                        ST val = (ST)0;
                        if (lo[r] < hi0[r] && doc_ids[lo[r]] == doc[r]) val = payload[lo[r]];
                        M[mpos[r]] = val;
                    }
                }
            }
            __syncthreads();
            for (int e = tid; e < ec; e += kThreads) {
                ST s = (ST)cs[e0 + e];
                for (int j = 0; j < nqc; ++j) s = s + M[e * ld + j];      // token order; + 0 for an absent token
                cs[e0 + e] = (double)s;
            }
            __syncthreads();
        }
    }
    __syncthreads();
}

// ---- short shape ---------------------------------------------------------------------------------------------------------------------
// grid = queries of the short shape (qsel), block = 256.  Static LDS: 16 + 8 + 24 KiB + the token table.
template <typename ST>
__global__ __launch_bounds__(kThreads) void bm25_rows_short_kernel(
    const erh::ErhBm25RowsIndex ix, const int32_t *__restrict__ q_indptr, const int32_t *__restrict__ q_tok, const int32_t *__restrict__ rows,
    const int64_t *__restrict__ list_ptr, const int32_t *__restrict__ list_of, const int32_t *__restrict__ qsel, int k,
    int32_t *__restrict__ out_ids, double *__restrict__ out_sc, int32_t *__restrict__ out_len) {
    __shared__ double cs[kRowsCap];
    __shared__ int32_t ci[kRowsCap];
    __shared__ __attribute__((aligned(16))) char mraw[kMBytes];
    __shared__ TokTab tt;
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int b = qsel[blockIdx.x];
    const int l = list_of[b];
    const int64_t base = l < 0 ? 0 : list_ptr[l];
    int len = l < 0 ? 0 : (int)(list_ptr[l + 1] - base);
    if (len > kRowsCap) len = kRowsCap;                                  // (the host never sends a longer list here)
    const int qs = q_indptr[b], nq = q_indptr[b + 1] - qs;
    const int32_t *lr = rows + base;
    if (nq <= 0) len = 0;                                                // an empty query scores nothing
    if (tid == 0) s_n = 0;
    bm_rows_sums<ST>(ix, q_tok, qs, nq, lr, len, cs, reinterpret_cast<ST *>(mraw), &tt);
    // the positive rows, compacted in place: every thread takes its sums to registers first
    constexpr int PER = kRowsCap / kThreads;
    double v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int i = tid + u * kThreads; v[u] = i < len ? cs[i] : 0.0; }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = tid + u * kThreads;
        if (v[u] > 0.0) {
            const int at = atomicAdd(&s_n, 1);                           // (LDS slot only: the sort below fixes the order)
            cs[at] = v[u];
            ci[at] = lr[i];
        }
    }
    __syncthreads();
    const int n_pos = s_n;
    const int np2 = erh_next_pow2(n_pos < 2 ? 2 : n_pos);
    for (int i = n_pos + tid; i < np2; i += kThreads) { cs[i] = -INFINITY; ci[i] = 0x7fffffff; }
    erh_bitonic_rec_desc<double>(cs, ci, np2);                           // (begins and ends with a barrier)
    const int n = n_pos < k ? n_pos : k;
    const size_t orow = (size_t)b * k;
    for (int c = tid; c < k; c += kThreads) {
        out_ids[orow + c] = c < n ? ci[c] : -1;
        out_sc[orow + c] = c < n ? cs[c] : 0.0;
    }
    if (tid == 0) out_len[b] = n;
}

// ---- long shape ----------------------------------------------------------------------------------------------------------------------
// grid = work items of the chunk, block = 256: the widened scores of one segment of one query's list -> its span
template <typename ST>
__global__ __launch_bounds__(kThreads) void bm25_rows_score_kernel(
    const erh::ErhBm25RowsIndex ix, const int32_t *__restrict__ q_indptr, const int32_t *__restrict__ q_tok, const int32_t *__restrict__ rows,
    const int64_t *__restrict__ list_ptr, const int32_t *__restrict__ list_of, const erh::ErhBm25RowsItem *__restrict__ items,
    const int64_t *__restrict__ span_off, double *__restrict__ S64) {
    __shared__ double cs[kRowsCap];
    __shared__ __attribute__((aligned(16))) char mraw[kMBytes];
    __shared__ TokTab tt;
    const erh::ErhBm25RowsItem it = items[blockIdx.x];
    const int tid = threadIdx.x;
    const int b = it.q;
    const int n = it.n_rows < kRowsCap ? it.n_rows : kRowsCap;
    const int qs = q_indptr[b], nq = q_indptr[b + 1] - qs;
    const int32_t *lr = rows + list_ptr[list_of[b]] + it.i0;
    double *out = S64 + span_off[b] + it.i0;
    bm_rows_sums<ST>(ix, q_tok, qs, nq > 0 ? nq : 0, lr, n, cs, reinterpret_cast<ST *>(mraw), &tt);   // (no tokens: zeros)
    for (int i = tid; i < n; i += kThreads) out[i] = cs[i];
}

// grid = queries of the chunk (qord[0 .. grid)), block = 1024: span -> the top k of its POSITIVE scores, the list kept under an exact
// (score, id) threshold.  dense_rows_select_kernel's algorithm (dense_rows.hip) with the sparse route's rule that a score <= 0 is never
// returned: only positives are appended, so the fill level after the last shrink is the count that goes out.
__global__ __launch_bounds__(kSelectThreads) void bm25_rows_select_kernel(
    const double *__restrict__ S64, const int64_t *__restrict__ span_off, const int32_t *__restrict__ rows, const int64_t *__restrict__ list_ptr,
    const int32_t *__restrict__ list_of, const int32_t *__restrict__ qord, int k, int32_t *__restrict__ out_ids, double *__restrict__ out_sc,
    int32_t *__restrict__ out_len) {
    __shared__ double cs[kRowsCap];
    __shared__ int32_t ci[kRowsCap];
    __shared__ int s_n;
    __shared__ double s_tau;
    __shared__ int s_tau_idx, s_have_tau;
    const int tid = threadIdx.x;
    const int b = qord[blockIdx.x];
    const int l = list_of[b];
    const int64_t len = list_ptr[l + 1] - list_ptr[l];
    const int32_t *lr = rows + list_ptr[l];
    const double *row = S64 + span_off[b];
    if (tid == 0) { s_n = 0; s_have_tau = 0; s_tau = 0.0; s_tau_idx = 0; }
    __syncthreads();
    auto shrink = [&]() {                                                // uniform call: sort, keep k, refresh the threshold
        __syncthreads();
        const int n = s_n;
        const int np2 = erh_next_pow2(n < 2 ? 2 : n);
        for (int i = n + tid; i < np2; i += kSelectThreads) { cs[i] = -INFINITY; ci[i] = 0x7fffffff; }
        erh_bitonic_rec_desc<double>(cs, ci, np2);
        if (tid == 0) {
            s_n = n < k ? n : k;
            if (n >= k) { s_have_tau = 1; s_tau = cs[k - 1]; s_tau_idx = ci[k - 1]; }
        }
        __syncthreads();
    };
    for (int64_t p0 = 0; p0 < len; p0 += kSelectThreads) {
        // the fill level every thread decides on is read BETWEEN two barriers: without the second one a fast wave's appends of this step
        // would reach s_n before a slow wave has read it, and the waves would disagree on the (barrier-carrying) shrink
        const int fill = s_n;
        __syncthreads();
        if (fill > kRowsCap - kSelectThreads) shrink();                  // uniform: appends below always fit
        const int64_t p = p0 + tid;
        if (p < len) {
            const double s = row[p];
            const int32_t id = lr[p];
            if (s > 0.0 && (!s_have_tau || s > s_tau || (s == s_tau && id < s_tau_idx))) {
                const int at = atomicAdd(&s_n, 1);                       // (LDS slot only: the sort below fixes the order)
                cs[at] = s;
                ci[at] = id;
            }
        }
        __syncthreads();
    }
    shrink();
    const int n = s_n < k ? s_n : k;
    const size_t orow = (size_t)b * k;
    for (int i = tid; i < k; i += kSelectThreads) {
        out_ids[orow + i] = i < n ? ci[i] : -1;
        out_sc[orow + i] = i < n ? cs[i] : 0.0;
    }
    if (tid == 0) out_len[b] = n;
}

}  // namespace

namespace erh {

hipError_t bm25_rows_init() { return hipSuccess; }   // static LDS only (<= 49 KiB): no function attribute to raise

hipError_t launch_bm25_rows_short(const ErhBm25RowsIndex &ix, const int32_t *q_indptr, const int32_t *q_tok, const int32_t *rows,
                                  const int64_t *list_ptr, const int32_t *list_of, const int32_t *qsel, int n_q, int k, int32_t *out_ids,
                                  double *out_sc, int32_t *out_len, hipStream_t st) {
    if (n_q <= 0) return hipSuccess;
    if (k < 1 || k > kRowsCap) return hipErrorInvalidValue;
    if (ix.f64)
        hipLaunchKernelGGL(bm25_rows_short_kernel<double>, dim3((unsigned)n_q), dim3(kThreads), 0, st, ix, q_indptr, q_tok, rows, list_ptr, list_of,
                           qsel, k, out_ids, out_sc, out_len);
    else
        hipLaunchKernelGGL(bm25_rows_short_kernel<float>, dim3((unsigned)n_q), dim3(kThreads), 0, st, ix, q_indptr, q_tok, rows, list_ptr, list_of,
                           qsel, k, out_ids, out_sc, out_len);
    return hipGetLastError();
}

hipError_t launch_bm25_rows_score(const ErhBm25RowsIndex &ix, const int32_t *q_indptr, const int32_t *q_tok, const int32_t *rows,
                                  const int64_t *list_ptr, const int32_t *list_of, const ErhBm25RowsItem *items, int n_items,
                                  const int64_t *span_off, double *S64, hipStream_t st) {
    if (n_items <= 0) return hipSuccess;
    if (ix.f64)
        hipLaunchKernelGGL(bm25_rows_score_kernel<double>, dim3((unsigned)n_items), dim3(kThreads), 0, st, ix, q_indptr, q_tok, rows, list_ptr,
                           list_of, items, span_off, S64);
    else
        hipLaunchKernelGGL(bm25_rows_score_kernel<float>, dim3((unsigned)n_items), dim3(kThreads), 0, st, ix, q_indptr, q_tok, rows, list_ptr,
                           list_of, items, span_off, S64);
    return hipGetLastError();
}

hipError_t launch_bm25_rows_select(const double *S64, const int64_t *span_off, const int32_t *rows, const int64_t *list_ptr,
                                   const int32_t *list_of, const int32_t *qord, int n_q, int k, int32_t *out_ids, double *out_sc,
                                   int32_t *out_len, hipStream_t st) {
    if (n_q <= 0) return hipSuccess;
    if (k < 1 || k > kSelectThreads) return hipErrorInvalidValue;        // the list must hold k survivors + one step of appends
    hipLaunchKernelGGL(bm25_rows_select_kernel, dim3((unsigned)n_q), dim3(kSelectThreads), 0, st, S64, span_off, rows, list_ptr, list_of, qord,
                       k, out_ids, out_sc, out_len);
    return hipGetLastError();
}

}  // namespace erh
