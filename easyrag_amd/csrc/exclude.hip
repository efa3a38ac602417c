// Exclude lists (erh_dense_topk_excl / erh_bm25_topk_excl, exclude_entries.hip; DESIGN K12): query b ranks what it may see EXCEPT the ids
// of its exclusion list.  The route's own pipeline runs unchanged at depth kk = k + (longest exclusion list of the call), and this kernel
// removes the excluded ids from each over-fetched list, in order, and keeps the first k.
//
// Why that is exact: at most e_b <= kk - k entries leave query b's list of the top kk, so -- when the allowed population holds kk rows or
// more -- at least k survive, and the first k survivors are the top k of (allowed \ excluded) under the same order: a row of that top k
// has fewer than k non-excluded rows in front of it, hence fewer than k + e_b rows in all, so it is in the longer list.  When the list is
// shorter than kk it holds every row the query can see, and its survivors are all there is.  The score > 0 cut of the sparse route is a
// property of the document alone and survives the removal; every survivor keeps its score bits (copied, never recomputed) and its place
// relative to the other survivors, so the canonical order (score descending, id ascending) does too.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kDropThreads = 256;
constexpr int kDropWaves = kDropThreads / 64;

// One workgroup per query b.  in_ids / in_sc [B x kk], in_len[b] valid entries; the exclusion list excl_ids[excl_ptr[b] .. excl_ptr[b + 1])
// is strictly ascending (checked on the host).  Entries are taken kDropThreads at a time, in list order: a thread binary-searches its id in
// the exclusion range, the survivors' places come from the wave ballot (v_mbcnt: survivors in the lanes below) plus the totals of the
// waves in front (LDS) plus the survivors of the rounds before.  The first k go to out row b, the rest of the row is padded with id -1 /
// score 0, out_len[b] = min(k, survivors).  Scores travel as 64-bit words.  No atomics, no data-dependent order: deterministic.
__global__ __launch_bounds__(kDropThreads) void topk_drop_kernel(const int32_t *__restrict__ in_ids, const unsigned long long *__restrict__ in_sc,
                                                                 const int32_t *__restrict__ in_len, int kk, const int32_t *__restrict__ excl_ptr,
                                                                 const int32_t *__restrict__ excl_ids, int k, int32_t *__restrict__ out_ids,
                                                                 unsigned long long *__restrict__ out_sc, int32_t *__restrict__ out_len) {
    __shared__ int s_wave[kDropWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t irow = (size_t)b * kk, orow = (size_t)b * k;
    const int n = min(max(in_len[b], 0), kk);
    const int e0 = excl_ptr[b], e1 = excl_ptr[b + 1];
    if (e1 <= e0) {                                       // nothing excluded: a truncating copy (workgroup-uniform)
        const int l = min(n, k);
        for (int c = tid; c < k; c += kDropThreads) {
            const bool in = c < l;
            out_ids[orow + c] = in ? in_ids[irow + c] : -1;
            out_sc[orow + c] = in ? in_sc[irow + c] : 0ull;
        }
        if (tid == 0) out_len[b] = l;
        return;
    }
    int base = 0;                                         // survivors of the rounds so far (the same in every thread)
    for (int i0 = 0; i0 < n && base < k; i0 += kDropThreads) {
        const int i = i0 + tid;
        bool keep = i < n;
        int32_t id = -1;
        if (keep) {
            id = in_ids[irow + i];
            int lo = e0, hi = e1;                         // first entry >= id
            while (lo < hi) { const int m = (lo + hi) >> 1; if (excl_ids[m] < id) lo = m + 1; else hi = m; }
            keep = !(lo < e1 && excl_ids[lo] == id);
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int front = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kDropWaves; ++w) { const int c = s_wave[w]; front += w < wave ? c : 0; total += c; }
        const int pos = base + front + rank;
        if (keep && pos < k) { out_ids[orow + pos] = id; out_sc[orow + pos] = in_sc[irow + i]; }
        base += total;
        __syncthreads();                                  // s_wave is rewritten by the next round
    }
    const int l = min(base, k);
    for (int c = l + tid; c < k; c += kDropThreads) { out_ids[orow + c] = -1; out_sc[orow + c] = 0ull; }
    if (tid == 0) out_len[b] = l;
}

}  // namespace

namespace erh {

hipError_t launch_topk_drop(const int32_t *in_ids, const double *in_sc, const int32_t *in_len, int kk, const int32_t *excl_ptr,
                            const int32_t *excl_ids, int B, int k, int32_t *out_ids, double *out_sc, int32_t *out_len, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (k < 1 || kk < k || kk > kTopkDropMaxDepth) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_drop_kernel, dim3((unsigned)B), dim3(kDropThreads), 0, st, in_ids, reinterpret_cast<const unsigned long long *>(in_sc),
                       in_len, kk, excl_ptr, excl_ids, k, out_ids, reinterpret_cast<unsigned long long *>(out_sc), out_len);
    return hipGetLastError();
}

}  // namespace erh
