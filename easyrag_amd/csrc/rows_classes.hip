// Row lists -> a CALL-LOCAL CLASS COLUMN (erh_dense_topk_rows / erh_bm25_topk_rows, the scan route of their long lists; DESIGN K11).
//
// A long list is a class that the handle's class column does not happen to hold, and several overlapping long lists cut the rows into
// CELLS: a cell is the set of rows with the same membership signature -- bit l of a row's 64-bit word says "in routed list l".  Cells are
// disjoint, every routed list is a union of cells, so a query on list l is the set filter {cells whose signature has bit l} and the sets
// pipelines (dense_sets.hip / bm25_sets.hip: exact top k per class, one merge) answer it exactly.
//
// Four small launches, all bounded by N or by the table:
//   rows_sig_kernel      every entry of routed list l ORs bit l into its row's word (vector atomics on global memory; the words were cleared)
//   rows_cells_kernel    every row with a non-zero word finds or claims the slot of its signature in an open-addressing table (compare-and-
//                        swap on the 64-bit key; linear probing) and adds itself to the slot's row count, first row and last row + 1.  The
//                        lanes of a wave that hold the same signature send ONE lane: a single list of 500 000 rows is one signature, and
//                        500 000 atomics on one address would be the kernel.
//   rows_number_kernel   every occupied slot draws the next cell number and writes the cell's record behind the header
//   rows_column_kernel   every row looks its signature up (the keys no longer change) and writes its cell number into the int16 column, -1
//                        for a row in no routed list
// The numbering follows the arrival order of the draws, so it differs from run to run; the merged result does not depend on it (a cell's list
// is the same whatever its number, and the merge orders by (score, row id)).  A table that fills up, or more cells than the column can number,
// sets the overflow word / is seen in the cell count: the host then answers the call on the row-by-row shapes.
//   Giving up is cheap: rows_cells_kernel counts the slots it claims and raises the overflow word with the claim that exceeds max_cells, so the
// table never fills beyond half (slots >= 2 * (max_cells + 1)); a probe sequence ends after kProbeMax slots (at load 1/2 a run that long
// does not occur; reaching it counts as overflow, which is always safe: the call is answered on the row-by-row shapes); and once the word
// is up no row probes again -- waves leave at entry, leaders skip their probe, rows_column_kernel returns (the host discards the column).
// A call of 20 random half-corpus lists over 1M rows has about 600 000 signatures: it stops after max_cells claims, not after 4e10 probes.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kNoSlot = -1;
constexpr int kProbeMax = 256;

struct Table {
    uint32_t *hdr;                 // [0] cells, [1] overflow, [2] slots claimed
    erh::ErhRowsCell *cells;       // [max_cells]
    unsigned long long *keys;      // [slots], 0 = free (a signature is never 0)
    int32_t *cnt, *nlo, *hi, *num; // [slots] each: rows, INT32_MAX - first row, last row + 1, cell number
};

__host__ __device__ inline Table table_of(void *base, int slots, int max_cells) {
    Table t;
    char *p = reinterpret_cast<char *>(base);
    t.hdr = reinterpret_cast<uint32_t *>(p);
    t.cells = reinterpret_cast<erh::ErhRowsCell *>(p + 16);
    p += 16 + (size_t)max_cells * sizeof(erh::ErhRowsCell);
    t.keys = reinterpret_cast<unsigned long long *>(p);
    p += (size_t)slots * 8;
    t.cnt = reinterpret_cast<int32_t *>(p);
    t.nlo = t.cnt + slots;
    t.hi = t.nlo + slots;
    t.num = t.hi + slots;
    return t;
}

__device__ __forceinline__ bool overflowed(const Table &t) {
    return __hip_atomic_load(&t.hdr[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

__device__ __forceinline__ uint32_t sig_hash(unsigned long long s, int slots) {
    return (uint32_t)((s * 0x9E3779B97F4A7C15ull) >> 40) & (uint32_t)(slots - 1);
}

// grid = (blocks, routed lists), block = 256
__global__ __launch_bounds__(kThreads) void rows_sig_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ routed, int64_t N,
                                                            unsigned long long *__restrict__ sig) {
    const int l = blockIdx.y;
    const int64_t off = routed[2 * l], len = routed[2 * l + 1];
    const unsigned long long bit = 1ull << l;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < len; i += (int64_t)gridDim.x * kThreads) {
        const int32_t r = rows[off + i];
        if (r >= 0 && (int64_t)r < N) atomicOr(&sig[r], bit);             // (the host checked the rows; the bound costs nothing)
    }
}

// grid = ceil(N / 256), block = 256: one row per thread
__global__ __launch_bounds__(kThreads) void rows_cells_kernel(const unsigned long long *__restrict__ sig, int64_t N, int slots, int max_cells,
                                                              Table t) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (__ballot(overflowed(t)) != 0ull) return;                          // (wave-uniform: the whole wave leaves)
    const unsigned long long s = r < N ? sig[r] : 0ull;
    unsigned long long todo = __ballot(s != 0ull);
    while (todo) {                                                        // (wave-uniform: one signature of the wave per turn)
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lo32 = (uint32_t)__shfl((int)(uint32_t)s, leader), hi32 = (uint32_t)__shfl((int)(uint32_t)(s >> 32), leader);
        const unsigned long long ls = ((unsigned long long)hi32 << 32) | lo32;
        const unsigned long long same = __ballot(s == ls);
        if (lane == leader) {
            // rows ascend with the lane: the leader holds the group's first row, its highest lane the last
            const int n = __popcll(same), top = 63 - __clzll((long long)same);
            const int32_t first = (int32_t)r, last1 = (int32_t)(r - lane + top) + 1;
            uint32_t at = sig_hash(ls, slots);
            int slot = kNoSlot;
            bool over = overflowed(t);
            const int probes = slots < kProbeMax ? slots : kProbeMax;
            for (int probe = 0; !over && probe < probes; ++probe) {
                const unsigned long long was = atomicCAS(&t.keys[at], 0ull, ls);
                if (was == 0ull) over = atomicAdd(&t.hdr[2], 1u) >= (uint32_t)max_cells;   // (a claim beyond what the column can number)
                if (was == 0ull || was == ls) { slot = (int)at; break; }
                at = (at + 1) & (uint32_t)(slots - 1);
            }
            if (over || slot == kNoSlot) atomicOr(&t.hdr[1], 1u);
            else {
                atomicAdd(&t.cnt[slot], n);
                atomicMax(&t.nlo[slot], 2147483647 - first);
                atomicMax(&t.hi[slot], last1);
            }
        }
        todo &= ~same;
    }
}

// grid = ceil(slots / 256), block = 256
__global__ __launch_bounds__(kThreads) void rows_number_kernel(int slots, int max_cells, Table t) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= slots) return;
    const unsigned long long key = t.keys[s];
    if (key == 0ull) return;
    const uint32_t c = atomicAdd(&t.hdr[0], 1u);
    t.num[s] = (int32_t)c;
    if (c < (uint32_t)max_cells) t.cells[c] = erh::ErhRowsCell{key, t.cnt[s], 2147483647 - t.nlo[s], t.hi[s], 0};
}

// grid = ceil(N / 256), block = 256
__global__ __launch_bounds__(kThreads) void rows_column_kernel(const unsigned long long *__restrict__ sig, int64_t N, int slots, Table t,
                                                               int16_t *__restrict__ cls) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= N || overflowed(t)) return;                                 // (after an overflow the host discards the column)
    const unsigned long long s = sig[r];
    int c = -1;
    if (s != 0ull) {
        uint32_t at = sig_hash(s, slots);
        const int probes = slots < kProbeMax ? slots : kProbeMax;         // (rows_cells_kernel placed every key within as many)
        for (int probe = 0; probe < probes; ++probe) {
            const unsigned long long key = t.keys[at];
            if (key == s) { c = t.num[at]; break; }
            if (key == 0ull) break;
            at = (at + 1) & (uint32_t)(slots - 1);
        }
    }
    cls[r] = (c >= 0 && c <= erh::kRowsClassMax) ? (int16_t)c : (int16_t)-1;
}

}  // namespace

namespace erh {

int rows_classes_slots(int64_t max_cells) {
    int slots = 64;
    while (slots < 65536 && (int64_t)slots < 2 * (max_cells + 1)) slots <<= 1;
    return slots;
}

size_t rows_classes_table_bytes(int slots, int max_cells) {
    return 16 + (size_t)max_cells * sizeof(ErhRowsCell) + (size_t)slots * (8 + 4 * 4);
}

hipError_t launch_rows_classes(const int32_t *rows, const int64_t *routed, int n_routed, int64_t max_len, int64_t N, int slots, int max_cells,
                               unsigned long long *sig, void *table, int16_t *cls, hipStream_t st) {
    if (n_routed < 1 || n_routed > kRowsClassLists || N < 1 || N > 2147483647LL || max_len < 1 || max_cells < 1 || slots < 64 ||
        slots > 65536 || (slots & (slots - 1)) != 0)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(sig, 0, (size_t)N * 8, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(table, 0, rows_classes_table_bytes(slots, max_cells), st);
    if (e != hipSuccess) return e;
    const Table t = table_of(table, slots, max_cells);
    const unsigned per_row = (unsigned)((N + kThreads - 1) / kThreads);
    const unsigned per_list = (unsigned)std::min<int64_t>((max_len + kThreads - 1) / kThreads, 4096);
    hipLaunchKernelGGL(rows_sig_kernel, dim3(per_list, (unsigned)n_routed), dim3(kThreads), 0, st, rows, routed, N, sig);
    hipLaunchKernelGGL(rows_cells_kernel, dim3(per_row), dim3(kThreads), 0, st, sig, N, slots, max_cells, t);
    hipLaunchKernelGGL(rows_number_kernel, dim3((unsigned)((slots + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, slots, max_cells, t);
    hipLaunchKernelGGL(rows_column_kernel, dim3(per_row), dim3(kThreads), 0, st, sig, N, slots, t, cls);
    return hipGetLastError();
}

}  // namespace erh
