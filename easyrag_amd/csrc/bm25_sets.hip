// Sparse route with a SET of allowed classes per query (erh_bm25_topk_sets, api.hip): query b allowed to see the classes {c_1 .. c_m} is
// run as m ordinary single-class sub-queries (class-column batches through bm25_topk_dev: every scan arm, the dir tile range, the mixed
// launch and the exact-scan fall-back see an ordinary class column), and this kernel merges the m sub-lists into the top k of their union.
//
// Why the merge is exact: every document carries exactly one class, so the sub-queries of one query rank DISJOINT document sets whose
// union is the allowed set.  A member of the union's top k is, a fortiori, in the top k of its own class (fewer competitors there).  The
// score > 0 cut (ref retrievers.py:195-196) is a property of the document alone, so it commutes with the split.  Each sub-list holds the
// exact top k of its class in canonical order (score descending, then document id ascending), so the union's top k is the top k of the
// concatenated sub-lists, and a merge of canonical lists under the same order gives it.  Scores are copied, never recomputed: the merged
// list carries the scans' bits.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kMergeThreads = 256;
constexpr int kMergeMaxK = 1024;             // erh_bm25_topk's limit on k; 3 x 1024 x 12 B = 36 KiB of LDS: four workgroups per CU

// canonical order: a before b iff a.s > b.s, or a.s == b.s and a.id < b.id
__device__ __forceinline__ bool before(double as, int32_t ai, double bs, int32_t bi) {
    return as > bs || (as == bs && ai < bi);
}

// One workgroup per output query b: sub-lists sub_ptr[b] .. sub_ptr[b + 1] of [rows x k] (each canonical, sub_len[s] <= k entries) ->
// out row b, padded with id -1 / score 0.  Any number of sub-lists: a chain of two-list merges held in LDS (accumulator, next list,
// output), each a merge by rank -- an element's place in the merged list is its place in its own list plus the number of elements of the
// other list in front of it (binary search; on equal keys the accumulator's element goes first, so two places never coincide) --
// truncated to k.  An empty sub-list is skipped (a workgroup-uniform decision).  No atomics, no data-dependent scheduling: deterministic.
__global__ __launch_bounds__(kMergeThreads) void bm25_set_merge_kernel(const int32_t *__restrict__ sub_ids, const double *__restrict__ sub_sc,
                                                                      const int32_t *__restrict__ sub_len, const int32_t *__restrict__ sub_ptr,
                                                                      int k, int32_t *__restrict__ out_ids, double *__restrict__ out_sc,
                                                                      int32_t *__restrict__ out_len) {
    __shared__ double s_sc[3][kMergeMaxK];
    __shared__ int32_t s_id[3][kMergeMaxK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int s0 = sub_ptr[b], s1 = sub_ptr[b + 1];
    const size_t orow = (size_t)b * k;
    if (s1 - s0 == 1) {                                   // one sub-list: a copy (the padding written here, whatever the scan left behind it)
        const size_t irow = (size_t)s0 * k;
        const int l = min(max(sub_len[s0], 0), k);
        for (int c = tid; c < k; c += kMergeThreads) {
            const bool in = c < l;
            out_ids[orow + c] = in ? sub_ids[irow + c] : -1;
            out_sc[orow + c] = in ? sub_sc[irow + c] : 0.0;
        }
        if (tid == 0) out_len[b] = l;
        return;
    }
    int la = 0, acc = 0;                                  // accumulator: LDS buffer `acc`, la entries
    for (int s = s0; s < s1; ++s) {
        const int lb = min(max(sub_len[s], 0), k);
        if (lb == 0) continue;
        const size_t irow = (size_t)s * k;
        const int nxt = (acc + 1) % 3, out = (acc + 2) % 3;
        for (int c = tid; c < lb; c += kMergeThreads) { s_sc[nxt][c] = sub_sc[irow + c]; s_id[nxt][c] = sub_ids[irow + c]; }
        __syncthreads();
        for (int i = tid; i < la; i += kMergeThreads) {   // accumulator entries: + the next list's entries strictly in front
            const double v = s_sc[acc][i];
            const int32_t id = s_id[acc][i];
            int lo = 0, hi = lb;
            while (lo < hi) { const int m = (lo + hi) >> 1; if (before(s_sc[nxt][m], s_id[nxt][m], v, id)) lo = m + 1; else hi = m; }
            const int pos = i + lo;
            if (pos < k) { s_sc[out][pos] = v; s_id[out][pos] = id; }
        }
        for (int j = tid; j < lb; j += kMergeThreads) {   // next list's entries: + the accumulator's entries in front or equal
            const double v = s_sc[nxt][j];
            const int32_t id = s_id[nxt][j];
            int lo = 0, hi = la;
            while (lo < hi) { const int m = (lo + hi) >> 1; if (!before(v, id, s_sc[acc][m], s_id[acc][m])) lo = m + 1; else hi = m; }
            const int pos = j + lo;
            if (pos < k) { s_sc[out][pos] = v; s_id[out][pos] = id; }
        }
        __syncthreads();
        la = min(la + lb, k);
        acc = out;
    }
    for (int c = tid; c < k; c += kMergeThreads) {
        const bool in = c < la;
        out_ids[orow + c] = in ? s_id[acc][c] : -1;
        out_sc[orow + c] = in ? s_sc[acc][c] : 0.0;
    }
    if (tid == 0) out_len[b] = la;
}

}  // namespace

namespace erh {

hipError_t launch_bm25_set_merge(const int32_t *sub_ids, const double *sub_sc, const int32_t *sub_len, const int32_t *sub_ptr, int B, int k,
                                 int32_t *out_ids, double *out_sc, int32_t *out_len, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (k < 1 || k > kMergeMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bm25_set_merge_kernel, dim3((unsigned)B), dim3(kMergeThreads), 0, st, sub_ids, sub_sc, sub_len, sub_ptr, k, out_ids,
                       out_sc, out_len);
    return hipGetLastError();
}

}  // namespace erh
