// Dense route over EXPLICIT ROW LISTS (erh_dense_topk_rows, api.hip): query b ranks the rows of its list -- sorted, distinct row ids in the
// caller's numbering -- and nothing else.  A Qdrant search restricted to a point-id set, the dense twin of BM25Retriever.get_scores(query,
// docs), a dir of a few hundred chunks: wherever the allowed rows are few, scanning the matrix for them is the waste this file removes.
//
// Why it is exact: there is no threshold, no candidate budget and no speculation.  EVERY listed row gets the pinned-order fp64 score
// (select.hip: dense_exact_all_kernel / dense_finalize_kernel are the definition) -- lane j of a wave adds the products of
// the elements 512 t + 8 j + e one after the other (a product of two fp16 values is exact in fp32, and its sum with an fp64 accumulator
// is one rounding, fused or not), then the xor butterfly 32 .. 1 -- and the list is ranked by (score desc, row id asc).  The bits are those
// of every other EXACT entry of the library.
//
// Two shapes, chosen per query by the length of its list:
//   short (<= kRowsCap = 2048 rows)  ONE launch, one workgroup per query.  The four waves take the rows round-robin, two rows in flight per
//                                    wave, a row being one 16-byte load per lane and 512-element round; the query fragments sit in registers
//                                    (d <= 1024: two half8 per lane) or in LDS.  Scores and ids go to LDS (2048 x 12 bytes), one bitonic sort
//                                    of the next power of two of the list length, k entries out.
//   long  (any length up to N)       two launches per chunk of queries.  dense_rows_score_kernel: one workgroup per work item (list, group of up to
//                                    kRowsGroup queries THAT SHARE the list, segment of kRowsSeg rows) holds the group's queries in LDS, loads
//                                    every row of the segment once and writes kRowsGroup fp64 scores per row into the queries' spans of the score
//                                    buffer.  dense_rows_select_kernel: one workgroup per query streams its span through a 2048-entry list kept
//                                    under an exact (score, id) threshold -- dense_exact_select_kernel's algorithm over a span instead of a row
//                                    of S64.
// No atomics on results, no data-dependent scheduling between workgroups: deterministic.  Row ids are validated on the host ([0, N),
// strictly ascending) before anything is enqueued, so no gather can leave the matrix.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kRowsCap = erh::kDenseRowsShortMax;   // 2048: kExCap of the exhaustive select
constexpr int kRowsGroup = erh::kDenseRowsGroup;
constexpr int kShortThreads = 256;
constexpr int kScoreThreads = 256;
constexpr int kSelectThreads = 1024;

// the pinned inner step: 8 products of one 16-byte fragment, added in element order
__device__ __forceinline__ double rows_acc8(double acc, const half8 xv, const half8 qv) {
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = acc + (double)((float)xv[u] * (float)qv[u]);
    return acc;
}
__device__ __forceinline__ double rows_butterfly(double acc) {
    for (int o = 32; o >= 1; o >>= 1) acc = acc + __shfl_xor(acc, o);
    return acc;
}

// ---- short shape ---------------------------------------------------------------------------------------------------------------------
// grid = queries of the short shape (qsel), block = 256.  QR > 0: d <= 512 * QR, query fragments in registers; QR == 0: in dynamic LDS (d * 2
// bytes).  Static LDS: 24 KiB.
template <int QR>
__global__ __launch_bounds__(kShortThreads) void dense_rows_short_kernel(
    const _Float16 *__restrict__ X, int64_t N, int d, int64_t pos_mul, const _Float16 *__restrict__ Q16, const int32_t *__restrict__ rows,
    const int64_t *__restrict__ list_ptr, const int32_t *__restrict__ list_of, const int32_t *__restrict__ qsel, int k,
    int32_t *__restrict__ out_ids, double *__restrict__ out_sc, int32_t *__restrict__ out_len) {
    __shared__ double cs[kRowsCap];
    __shared__ int32_t ci[kRowsCap];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = qsel[blockIdx.x];
    const int l = list_of[b];
    const int64_t base = l < 0 ? 0 : list_ptr[l];
    int len = l < 0 ? 0 : (int)(list_ptr[l + 1] - base);
    if (len > kRowsCap) len = kRowsCap;                                  // (the host never sends a longer list here)
    const _Float16 *qrow = Q16 + (int64_t)b * d;
    half8 qr[QR > 0 ? QR : 1];
    if constexpr (QR > 0) {
#pragma unroll
        for (int t = 0; t < QR; ++t) {
            const int off = 512 * t + 8 * lane;
            if (off < d) qr[t] = *reinterpret_cast<const half8 *>(qrow + off);
            else qr[t] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    } else {
        for (int i = tid; i < d / 8; i += kShortThreads) reinterpret_cast<half8 *>(smem)[i] = reinterpret_cast<const half8 *>(qrow)[i];
        __syncthreads();
    }
    for (int i0 = wave; i0 < len; i0 += 8) {                             // rows i0 and i0 + 4 of the list: two gathers in flight per wave
        const int i1 = i0 + 4;
        const bool two = i1 < len;
        const int32_t o0 = rows[base + i0];
        const int32_t o1 = two ? rows[base + i1] : o0;
        const _Float16 *x0 = X + erh_mulmod(o0, pos_mul, N) * d;
        const _Float16 *x1 = X + erh_mulmod(o1, pos_mul, N) * d;
        double a0 = 0.0, a1 = 0.0;
        if constexpr (QR > 0) {
            half8 v0[QR], v1[QR];
#pragma unroll
            for (int t = 0; t < QR; ++t) {
                const int off = 512 * t + 8 * lane;
                if (off < d) {
                    v0[t] = *reinterpret_cast<const half8 *>(x0 + off);
                    v1[t] = *reinterpret_cast<const half8 *>(x1 + off);
                }
            }
#pragma unroll
            for (int t = 0; t < QR; ++t) {
                const int off = 512 * t + 8 * lane;
                if (off < d) { a0 = rows_acc8(a0, v0[t], qr[t]); a1 = rows_acc8(a1, v1[t], qr[t]); }
            }
        } else {
            for (int off = 8 * lane; off < d; off += 512) {
                const half8 v0 = *reinterpret_cast<const half8 *>(x0 + off);
                const half8 v1 = *reinterpret_cast<const half8 *>(x1 + off);
                const half8 qv = *reinterpret_cast<const half8 *>(reinterpret_cast<const _Float16 *>(smem) + off);
                a0 = rows_acc8(a0, v0, qv);
                a1 = rows_acc8(a1, v1, qv);
            }
        }
        a0 = rows_butterfly(a0);
        a1 = rows_butterfly(a1);
        if (lane == 0) {
            cs[i0] = a0; ci[i0] = o0;
            if (two) { cs[i1] = a1; ci[i1] = o1; }
        }
    }
    const int np2 = erh_next_pow2(len < 2 ? 2 : len);
    for (int i = len + tid; i < np2; i += kShortThreads) { cs[i] = -INFINITY; ci[i] = 0x7fffffff; }
    erh_bitonic_rec_desc<double>(cs, ci, np2);                           // (barriers inside: the scores above are visible)
    const int n = len < k ? len : k;
    const size_t orow = (size_t)b * k;
    for (int c = tid; c < k; c += kShortThreads) {
        out_ids[orow + c] = c < n ? ci[c] : -1;
        out_sc[orow + c] = c < n ? cs[c] : 0.0;
    }
    if (tid == 0) out_len[b] = n;
}

// ---- long shape ----------------------------------------------------------------------------------------------------------------------
// grid = work items of the chunk, block = 256 (4 waves), dynamic LDS = kRowsGroup * d * 2 bytes.  Two rows in flight per wave.
__global__ __launch_bounds__(kScoreThreads) void dense_rows_score_kernel(
    const _Float16 *__restrict__ X, int64_t N, int d, int64_t pos_mul, const _Float16 *__restrict__ Q16, const int32_t *__restrict__ rows,
    const erh::ErhRowsItem *__restrict__ items, const int32_t *__restrict__ qord, const int64_t *__restrict__ span_off,
    double *__restrict__ S64) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int64_t s_span[kRowsGroup];
    _Float16 *qs = reinterpret_cast<_Float16 *>(smem);
    const erh::ErhRowsItem it = items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = it.nq;
    const int vec = d / 8;
    for (int i = tid; i < ng * vec; i += kScoreThreads) {
        const int g = i / vec, o = i - g * vec;
        reinterpret_cast<half8 *>(qs)[(size_t)g * vec + o] = reinterpret_cast<const half8 *>(Q16 + (int64_t)qord[it.q_at + g] * d)[o];
    }
    if (tid < ng) s_span[tid] = span_off[qord[it.q_at + tid]] + it.i0;
    __syncthreads();
    const int32_t *lr = rows + it.row_off;
    for (int r0 = wave; r0 < it.n_rows; r0 += 8) {
        const int r1 = r0 + 4;
        const bool two = r1 < it.n_rows;
        const _Float16 *x0 = X + erh_mulmod(lr[r0], pos_mul, N) * d;
        const _Float16 *x1 = X + erh_mulmod(lr[two ? r1 : r0], pos_mul, N) * d;
        double a0[kRowsGroup], a1[kRowsGroup];
#pragma unroll
        for (int g = 0; g < kRowsGroup; ++g) { a0[g] = 0.0; a1[g] = 0.0; }
        for (int off = 8 * lane; off < d; off += 512) {
            const half8 v0 = *reinterpret_cast<const half8 *>(x0 + off);
            const half8 v1 = *reinterpret_cast<const half8 *>(x1 + off);
#pragma unroll
            for (int g = 0; g < kRowsGroup; ++g) {
                if (g < ng) {
                    const half8 qv = *reinterpret_cast<const half8 *>(qs + (size_t)g * d + off);
                    a0[g] = rows_acc8(a0[g], v0, qv);
                    a1[g] = rows_acc8(a1[g], v1, qv);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < kRowsGroup; ++g) { a0[g] = rows_butterfly(a0[g]); a1[g] = rows_butterfly(a1[g]); }
        if (lane == 0) {
#pragma unroll
            for (int g = 0; g < kRowsGroup; ++g)
                if (g < ng) {
                    S64[s_span[g] + r0] = a0[g];
                    if (two) S64[s_span[g] + r1] = a1[g];
                }
        }
    }
}

// grid = queries of the chunk (qord[0 .. grid)), block = 1024: span -> top k, the list kept under an exact (score, id) threshold.
__global__ __launch_bounds__(kSelectThreads) void dense_rows_select_kernel(
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
            if (!s_have_tau || s > s_tau || (s == s_tau && id < s_tau_idx)) {
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

size_t dense_rows_score_lds(int d) { return (size_t)kRowsGroup * d * 2; }

hipError_t dense_rows_init() {
    // the score kernel's query block: up to 8 x d halves (d = 8192: 128 KiB, what one workgroup may take of a CU's 160 KiB)
    hipError_t e = hipFuncSetAttribute((const void *)dense_rows_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)dense_rows_short_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
}

hipError_t launch_dense_rows_short(const _Float16 *X, int64_t N, int d, int64_t pos_mul, const _Float16 *Q16, const int32_t *rows,
                                   const int64_t *list_ptr, const int32_t *list_of, const int32_t *qsel, int n_q, int k, int32_t *out_ids,
                                   double *out_sc, int32_t *out_len, hipStream_t st) {
    if (n_q <= 0) return hipSuccess;
    if (k < 1 || d % 8 != 0 || (size_t)d * 2 > 64 * 1024) return hipErrorInvalidValue;
#define ERH_ROWS_SHORT(QR, LDS)                                                                                                        \
    hipLaunchKernelGGL(dense_rows_short_kernel<QR>, dim3((unsigned)n_q), dim3(kShortThreads), LDS, st, X, N, d, pos_mul, Q16, rows, list_ptr, \
                       list_of, qsel, k, out_ids, out_sc, out_len)
    if (d <= 512) ERH_ROWS_SHORT(1, 0);
    else if (d <= 1024) ERH_ROWS_SHORT(2, 0);
    else ERH_ROWS_SHORT(0, (size_t)d * 2);
#undef ERH_ROWS_SHORT
    return hipGetLastError();
}

hipError_t launch_dense_rows_score(const _Float16 *X, int64_t N, int d, int64_t pos_mul, const _Float16 *Q16, const int32_t *rows,
                                   const ErhRowsItem *items, int n_items, const int32_t *qord, const int64_t *span_off, double *S64,
                                   hipStream_t st) {
    if (n_items <= 0) return hipSuccess;
    if (d % 8 != 0 || dense_rows_score_lds(d) > 128 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dense_rows_score_kernel, dim3((unsigned)n_items), dim3(kScoreThreads), dense_rows_score_lds(d), st, X, N, d, pos_mul,
                       Q16, rows, items, qord, span_off, S64);
    return hipGetLastError();
}

hipError_t launch_dense_rows_select(const double *S64, const int64_t *span_off, const int32_t *rows, const int64_t *list_ptr,
                                    const int32_t *list_of, const int32_t *qord, int n_q, int k, int32_t *out_ids, double *out_sc,
                                    int32_t *out_len, hipStream_t st) {
    if (n_q <= 0) return hipSuccess;
    if (k < 1 || k > kSelectThreads) return hipErrorInvalidValue;        // the list must hold k survivors + one step of appends
    hipLaunchKernelGGL(dense_rows_select_kernel, dim3((unsigned)n_q), dim3(kSelectThreads), 0, st, S64, span_off, rows, list_ptr, list_of, qord,
                       k, out_ids, out_sc, out_len);
    return hipGetLastError();
}

}  // namespace erh
