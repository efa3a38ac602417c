// Corpus-sharded layout (erh_shard_merge_topk / erh_shard_rrf, api.hip; easyrag_amd/dist.py: CorpusShards): every rank holds a
// contiguous slice of the corpus, answers ALL queries on it, and the ranks all-gather their packed top-k rows (fuse.hip:
// pack_topk_kernel).  This kernel turns what the gather delivers -- for rank r, n_queries rows [k x f64 score | k x i32 id | i32 len],
// rank after rank -- into the global top k, reading the packed rows where they lie (no unpack pass).
//
// Why the merge is exact: a document's score depends on (query, document) only, not on which other documents the handle holds; the
// slices are disjoint and cover the corpus, so a member of the global top k is in the top k of its own slice (fewer competitors
// there); every rank's list is canonical (score descending, then id ascending) and contiguous slices keep that order after the
// slice's first row is added to the ids.  The global list is therefore the canonical top k of the concatenated lists.  Scores are
// copied, never recomputed: the merged list carries the ranks' bits.
//
// One workgroup per query.  All live entries go to LDS (12 bytes each, list r at slot r * k), then a merge by rank: an entry's place in
// the merged list is its place in its own list plus, for every other list, the number of that list's entries in front of it (binary
// search).  The order is total -- (score desc, global id asc, rank asc) -- so no two entries share a place, whatever the caller's
// id_base; places < k are written straight to the output row.  No atomics on the data path, no data-dependent scheduling.
//   LDS: world * (12 k + 4) bytes -- 8 x 288: 27 KiB (five workgroups per CU), 8 x 1024: 96 KiB (one); the launcher refuses what does
//   not fit the CU's 160 KiB.  Packed rows are 8-byte aligned only (topk_row_bytes rounds 12 k + 4 up to 8): scores are read with
//   8-byte loads, ids with 4-byte loads, both coalesced along the list.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kShardThreads = 256;
constexpr size_t kShardLdsMax = 160 * 1024;          // LDS of one gfx950 CU: the largest single workgroup

struct ShardBases { int32_t v[erh::kShardMaxWorld]; };

__host__ __device__ inline size_t shard_lds_bytes(int world, int k) { return (size_t)world * k * 12 + (size_t)world * 4; }

// a in front of b in the total order; ra / rb are the ranks the entries came from
__device__ __forceinline__ bool in_front(double as, int32_t ai, int ra, double bs, int32_t bi, int rb) {
    return as > bs || (as == bs && (ai < bi || (ai == bi && ra < rb)));
}

// id_limit: global ids must lie in [0, id_limit) (the fusion behind this kernel indexes content_id with them); a list ends in front
// of its first id outside it -- a caller error (wrong id_base, rows that are not packed lists) never becomes a read out of bounds.
__global__ __launch_bounds__(kShardThreads) void shard_merge_kernel(const char *__restrict__ rows, int n_queries, int world, int k,
                                                                   int row_bytes, ShardBases base, int32_t id_limit,
                                                                   int32_t *__restrict__ out_ids, double *__restrict__ out_sc /* or null */,
                                                                   int32_t *__restrict__ out_len) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *s_sc = reinterpret_cast<double *>(smem);                       // [world][k]
    int32_t *s_id = reinterpret_cast<int32_t *>(s_sc + (size_t)world * k);  // [world][k]
    int32_t *s_len = s_id + (size_t)world * k;                             // [world]
    const int q = blockIdx.x, tid = threadIdx.x;
    for (int r = tid; r < world; r += kShardThreads) {
        const char *row = rows + ((size_t)r * n_queries + q) * row_bytes;
        const int l = reinterpret_cast<const int32_t *>(row + (size_t)k * 8)[k];
        s_len[r] = min(max(l, 0), k);
    }
    __syncthreads();
    for (int r = 0; r < world; ++r) {
        const char *row = rows + ((size_t)r * n_queries + q) * row_bytes;
        const double *i_sc = reinterpret_cast<const double *>(row);
        const int32_t *i_id = reinterpret_cast<const int32_t *>(row + (size_t)k * 8);
        const int l = s_len[r];
        const int64_t b = base.v[r];
        for (int i = tid; i < l; i += kShardThreads) {
            const int64_t g = (int64_t)i_id[i] + b;
            s_sc[(size_t)r * k + i] = i_sc[i];
            s_id[(size_t)r * k + i] = (int32_t)g;
            if (g < 0 || g >= (int64_t)id_limit) atomicMin(&s_len[r], i);
        }
    }
    __syncthreads();
    int total = 0;
    for (int r = 0; r < world; ++r) total += s_len[r];
    const int kk = min(total, k);
    const size_t orow = (size_t)q * k;
    for (int e = tid; e < world * k; e += kShardThreads) {
        const int r = e / k, i = e - r * k;
        if (i >= s_len[r]) continue;
        const double v = s_sc[e];
        const int32_t id = s_id[e];
        int pos = i;
        for (int o = 0; o < world && pos < k; ++o) {
            if (o == r) continue;
            const double *o_sc = s_sc + (size_t)o * k;
            const int32_t *o_id = s_id + (size_t)o * k;
            int lo = 0, hi = min(s_len[o], k - pos);                       // more than k - pos in front: the entry is out anyway
            while (lo < hi) {
                const int m = (lo + hi) >> 1;
                if (in_front(o_sc[m], o_id[m], o, v, id, r)) lo = m + 1; else hi = m;
            }
            pos += lo;
        }
        if (pos < k) {
            out_ids[orow + pos] = id;
            if (out_sc) out_sc[orow + pos] = v;
        }
    }
    for (int c = kk + tid; c < k; c += kShardThreads) {                    // padding as everywhere: id -1, score 0
        out_ids[orow + c] = -1;
        if (out_sc) out_sc[orow + c] = 0.0;
    }
    if (tid == 0) out_len[q] = kk;
}

}  // namespace

namespace erh {

bool shard_merge_fits(int world, int k) {
    return world >= 1 && world <= kShardMaxWorld && k >= 1 && k <= kShardMaxK && shard_lds_bytes(world, k) <= kShardLdsMax;
}

hipError_t shard_merge_init() {
    return hipFuncSetAttribute((const void *)shard_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kShardLdsMax);
}

hipError_t launch_shard_merge(const void *rows, int n_queries, int world, int k, const int32_t *id_base_host, int32_t id_limit,
                              int32_t *out_ids, double *out_sc, int32_t *out_len, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (!shard_merge_fits(world, k)) return hipErrorInvalidValue;
    ShardBases base;
    for (int r = 0; r < kShardMaxWorld; ++r) base.v[r] = r < world ? id_base_host[r] : 0;
    hipLaunchKernelGGL(shard_merge_kernel, dim3((unsigned)n_queries), dim3(kShardThreads), shard_lds_bytes(world, k), st,
                       (const char *)rows, n_queries, world, k, topk_row_bytes(k), base, id_limit, out_ids, out_sc, out_len);
    return hipGetLastError();
}

}  // namespace erh
