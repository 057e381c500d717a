// tpe_pool.hip -- a resident pool of whole configurations and its ranking
// under the current posterior (include/hyperopt_tpe.h, tpe_pool_*).
//
// The acquisition of a configuration is log l(x) - log g(x) of the
// tree-structured product densities (hyperopt/tpe.py:651-739 builds one
// below/above pair per label; broadcast_best :769-778 ranks by their
// difference): the sum over its active labels of lpdf_below - lpdf_above, a
// joint group's ll - lg standing in for its labels' terms.
//
// Layout in HBM (per context, kept across posterior rebuilds):
//   vals   : double[n_cols][n]             the pool, column-major, NaN = inactive
// Per tpe_pool_rank:
//   lb, la : double[n_cols + n_groups][n]  the lpdf planes (NaN: inactive / covered)
//   score  : double[n]
//   key    : uint64[n], idx : uint32[n]    order_key(score) (0: taken), entry
// Kernels
//   k_pool_dense   (entry tile, dense label)      k_round<double, DENSE_*, false>'s factor
//   k_pool_quant   (entry tile, quantized label)  quant_bounds / quant_lpdf, once per
//                  distinct value of a column on a grid (k_pool_spread: to the entries)
//   k_pool_cat     (entry tile, categorical label) the log p table
//   k_pool_gather  a group's columns -> [n][D]    (the joint score kernels read it)
//   k_pool_group   the joint lpdfs -> the group's plane
//   k_pool_sum     per entry: terms added left to right -> score, key, index
//   hipcub stable descending radix sort of (key, index), k_pool_top reads the head
// Per tpe_pool_draw (TPE's draw on a finite pool: Gumbel top-m on log l, then
// the best l/g inside the drawn set), after the planes and k_pool_sum above:
//   lsum   : double[n]                     the working-space log l per entry
//   key, idx as above, per round: order_key(lsum + Gumbel) (0: not free)
//   k_pool_lsum    per entry: the below terms added in k_pool_sum's order
//   k_pool_key     (round, entry): the Philox word pair -> Gumbel noise -> key
//   the same sort; k_pool_pick / k_pool_pick_final: (order_key(score), lowest
//                  index) over the first d sorted entries
//   k_pool_drawn   the drawn set to the caller's vector (diagnostics)
//   k_pool_take    one thread: the round's pick is not free for the next round
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"
#include "tpe_device.h"

using namespace tpe;
using namespace tpe_rt;

namespace {

constexpr int kPoolR = 4;                      // entries per thread, dense labels (k_round's kR)
constexpr int kPoolTile = kBlock * kPoolR;
constexpr size_t kPoolUniq = 4096;             // distinct values up to which a column is listed (uint16 positions)

// The value a lane scores: the entry's, or a harmless one for an inactive
// cell (NaN) and a lane past the pool -- 1 for an LGMM1 label, else 0, as
// draw_slots fills its idle slots.  Every lane runs the whole factor (the
// records are wave-uniform); its result is dropped for an inactive cell.
__device__ __forceinline__ double pool_value(const double* __restrict__ col, int64_t i, int64_t n, bool lgmm,
                                             bool& active) {
    double v = lgmm ? 1.0 : 0.0;
    active = false;
    if (i < n) {
        const double p = col[i];
        if (p == p) {
            v = p;
            active = true;
        }
    }
    return v;
}

// a covered column (its group supplies the term): NaN in both planes
__device__ __forceinline__ bool pool_covered(const int32_t* __restrict__ cover, int li, int64_t i0, int64_t n,
                                             int per_block, double* __restrict__ lb, double* __restrict__ la) {
    if (cover[li] < 0) return false;
    const double nan = __builtin_nan("");
    for (int64_t i = i0 + threadIdx.x; i < n && i < i0 + per_block; i += kBlock) {
        lb[(size_t)li * n + i] = nan;
        la[(size_t)li * n + i] = nan;
    }
    return true;
}

// Dense GMM1 / LGMM1 labels: grid (entry tiles, dense labels), the body of
// k_round<double, DENSE_*, false, R> without its maxloc.
__global__ __launch_bounds__(kBlock) void k_pool_dense(const DLabel* __restrict__ labels,
                                                       const int32_t* __restrict__ group,
                                                       const Comp<double>* __restrict__ comps,
                                                       const double* __restrict__ vals, int64_t n,
                                                       const int32_t* __restrict__ cover, double* __restrict__ out_lb,
                                                       double* __restrict__ out_la) {
    constexpr int R = kPoolR;
    const int li = group[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * kPoolTile;
    if (pool_covered(cover, li, i0, n, kPoolTile, out_lb, out_la)) return;   // (uniform over the workgroup)
    const DLabel L = labels[li];
    __shared__ double exp_tab[kExpTabSize];
    load_exp_table(exp_tab);
    const bool lgmm = L.mode == DENSE_LGMM;
    const double* col = vals + (size_t)li * n;
    double y[R], lb[R], la[R];
    bool active[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double x = pool_value(col, i0 + r * kBlock + threadIdx.x, n, lgmm, active[r]);
        y[r] = lgmm ? flog(x) : x;
    }
    lse_dense<R>(comps + L.comp_b, L.nb, L.shift_b, L.centre, y, lb, exp_tab);
    lse_dense<R>(comps + L.comp_a, L.na, L.shift_a, L.centre, y, la, exp_tab);
    if (lgmm) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lb[r] -= y[r];
            la[r] -= y[r];
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = i0 + r * kBlock + threadIdx.x;
        if (i < n) {
            out_lb[(size_t)li * n + i] = active[r] ? lb[r] : nan;
            out_la[(size_t)li * n + i] = active[r] ? la[r] : nan;
        }
    }
}

// Quantized labels: grid (entry tiles of kBlock, labels of the family); error
// bit 2 as k_round raises it (a negative upper end under an LGMM1 label).
// A column with few distinct values (PoolState::uoff: a grid) is scored once
// per distinct value -- entries [0, ucnt) of its list uvals + uoff into the
// tables ut_lb / ut_la, by the same function, so every entry gets the bits it
// would get on its own -- and k_pool_spread copies them to the entries.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_pool_quant(const DLabel* __restrict__ labels,
                                                       const int32_t* __restrict__ group,
                                                       const Comp<double>* __restrict__ comps64,
                                                       const double* __restrict__ vals, int64_t n,
                                                       const int32_t* __restrict__ cover,
                                                       const int32_t* __restrict__ uoff,
                                                       const int32_t* __restrict__ ucnt,
                                                       const double* __restrict__ uvals, double* __restrict__ ut_lb,
                                                       double* __restrict__ ut_la, double* __restrict__ out_lb,
                                                       double* __restrict__ out_la, int32_t* __restrict__ err) {
    const int li = group[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * kBlock;
    if (pool_covered(cover, li, i0, n, kBlock, out_lb, out_la)) return;
    const bool tab = uoff[li] >= 0;
    const int64_t m = tab ? ucnt[li] : n;
    if (i0 >= m) return;
    const DLabel L = labels[li];
    const int64_t i = i0 + threadIdx.x;
    bool active;
    const double x = pool_value(tab ? uvals + uoff[li] : vals + (size_t)li * n, i, m, MODE == QUANT_LGMM, active);
    double ub, lo;
    bool neg;
    quant_bounds<MODE>(L, x, ub, lo, neg);
    if (active && neg) atomicOr(err, 2);
    const double lb = quant_lpdf<MODE == QUANT_LGMM>(comps64 + L.comp_b, L.nb, ub, lo, L.logpacc_b);
    const double la = quant_lpdf<MODE == QUANT_LGMM>(comps64 + L.comp_a, L.na, ub, lo, L.logpacc_a);
    if (i < m) {
        const double nan = __builtin_nan("");
        double* dlb = tab ? ut_lb + uoff[li] : out_lb + (size_t)li * n;
        double* dla = tab ? ut_la + uoff[li] : out_la + (size_t)li * n;
        dlb[i] = active ? lb : nan;
        dla[i] = active ? la : nan;
    }
}

// the tables of k_pool_quant to the entries: umap (per listed column, at its
// slot uslot) holds each entry's position in the column's list
__global__ __launch_bounds__(kBlock) void k_pool_spread(const int32_t* __restrict__ group,
                                                        const double* __restrict__ vals, int64_t n,
                                                        const int32_t* __restrict__ cover,
                                                        const int32_t* __restrict__ uoff,
                                                        const int32_t* __restrict__ uslot,
                                                        const uint16_t* __restrict__ umap,
                                                        const double* __restrict__ ut_lb,
                                                        const double* __restrict__ ut_la, double* __restrict__ out_lb,
                                                        double* __restrict__ out_la) {
    const int li = group[blockIdx.y];
    if (cover[li] >= 0 || uoff[li] < 0) return;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double v = vals[(size_t)li * n + i];
    const double nan = __builtin_nan("");
    const int32_t at = uoff[li] + umap[(size_t)uslot[li] * n + i];
    out_lb[(size_t)li * n + i] = v == v ? ut_lb[at] : nan;
    out_la[(size_t)li * n + i] = v == v ? ut_la[at] : nan;
}

// Categorical labels: categorical_lpdf = log(p[sample]) (tpe.py:56-63); error
// bit 4 as k_round raises it (no integer in [0, upper)).
__global__ __launch_bounds__(kBlock) void k_pool_cat(const DLabel* __restrict__ labels,
                                                     const int32_t* __restrict__ group,
                                                     const Comp<double>* __restrict__ comps64,
                                                     const double* __restrict__ vals, int64_t n,
                                                     const int32_t* __restrict__ cover, double* __restrict__ out_lb,
                                                     double* __restrict__ out_la, int32_t* __restrict__ err) {
    const int li = group[blockIdx.y];
    const int64_t i0 = (int64_t)blockIdx.x * kBlock;
    if (pool_covered(cover, li, i0, n, kBlock, out_lb, out_la)) return;
    const DLabel L = labels[li];
    const int64_t i = i0 + threadIdx.x;
    if (i >= n) return;
    bool active;
    const double x = pool_value(vals + (size_t)li * n, i, n, false, active);
    const int64_t s = (int64_t)x;
    if (active && (s < 0 || s >= L.nb || (double)s != x)) atomicOr(err, 4);
    const int64_t sc = s < 0 ? 0 : (s >= L.nb ? L.nb - 1 : s);
    const double nan = __builtin_nan("");
    out_lb[(size_t)li * n + i] = active ? comps64[L.comp_b + sc].c : nan;
    out_la[(size_t)li * n + i] = active ? comps64[L.comp_a + sc].c : nan;
}

// One listed group: its columns cols[0 .. D) of the pool as the [n][D] array
// the joint score kernels read.  An entry with a NaN in any of them is
// inactive for the group: it is scored on harmless values (pool_value's) and
// k_pool_group drops the result.
__global__ __launch_bounds__(kBlock) void k_pool_gather(const DLabel* __restrict__ labels,
                                                        const double* __restrict__ vals, int64_t n,
                                                        const int32_t* __restrict__ cols, int32_t D,
                                                        double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    for (int d = 0; d < D; ++d) {
        const int c = cols[d];
        const int mode = labels[c].mode;
        bool active;
        out[(size_t)i * D + d] = pool_value(vals + (size_t)c * n, i, n, mode == DENSE_LGMM || mode == QUANT_LGMM,
                                            active);
    }
}

__global__ __launch_bounds__(kBlock) void k_pool_group(const double* __restrict__ vals, int64_t n,
                                                       const int32_t* __restrict__ cols, int32_t D,
                                                       const double* __restrict__ ll, const double* __restrict__ lg,
                                                       double* __restrict__ out_lb, double* __restrict__ out_la) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    bool active = true;
    for (int d = 0; d < D; ++d) {
        const double v = vals[(size_t)cols[d] * n + i];
        active &= v == v;
    }
    const double nan = __builtin_nan("");
    out_lb[i] = active ? ll[i] : nan;
    out_la[i] = active ? lg[i] : nan;
}

__global__ __launch_bounds__(kBlock) void k_pool_mark(const int64_t* __restrict__ taken, int64_t n_taken, int64_t n,
                                                      uint8_t* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_taken) return;
    const int64_t i = taken[t];
    if (i >= 0 && i < n) flag[i] = 1;   // (duplicates store the same byte)
}

// score[i]: from 0.0, the uncovered active columns' lb - la in ascending
// order, then the listed groups' in the order listed -- one thread per entry,
// so the sum reads nothing of the other entries.  key: order_key(score), 0 for
// a taken entry (below every score's key: order_key never returns 0).
__global__ __launch_bounds__(kBlock) void k_pool_sum(const double* __restrict__ vals, int64_t n, int32_t n_cols,
                                                     const int32_t* __restrict__ cover, int32_t n_groups,
                                                     const int32_t* __restrict__ goff,
                                                     const int32_t* __restrict__ gcols,
                                                     const double* __restrict__ lb, const double* __restrict__ la,
                                                     const uint8_t* __restrict__ taken, double* __restrict__ score,
                                                     uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < n_cols; ++c) {
        if (cover[c] >= 0) continue;
        const double v = vals[(size_t)c * n + i];
        if (v != v) continue;
        const double term = lb[(size_t)c * n + i] - la[(size_t)c * n + i];
        s += term;
    }
    for (int g = 0; g < n_groups; ++g) {
        bool active = true;
        for (int d = goff[g]; d < goff[g + 1]; ++d) {
            const double v = vals[(size_t)gcols[d] * n + i];
            active &= v == v;
        }
        if (!active) continue;
        const size_t row = (size_t)(n_cols + g) * n + i;
        const double term = lb[row] - la[row];
        s += term;
    }
    score[i] = s;
    key[i] = taken[i] ? 0ull : order_key(s);
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_pool_top(const uint32_t* __restrict__ idx, const double* __restrict__ score,
                                                     int32_t n_top, int64_t* __restrict__ top_i,
                                                     double* __restrict__ top_s) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_top) return;
    const uint32_t i = idx[j];
    top_i[j] = (int64_t)i;
    top_s[j] = score[i];
}

// lsum[i]: from 0.0, the below lpdfs in k_pool_sum's order, each in the
// label's working space -- a dense log label's lb is the document-space
// density (k_pool_dense subtracts log v), so its term is lb + flog(v); a
// group's is ll plus the flog(v) of its dense log columns, in the order the
// group lists them.
__global__ __launch_bounds__(kBlock) void k_pool_lsum(const DLabel* __restrict__ labels,
                                                      const double* __restrict__ vals, int64_t n, int32_t n_cols,
                                                      const int32_t* __restrict__ cover, int32_t n_groups,
                                                      const int32_t* __restrict__ goff,
                                                      const int32_t* __restrict__ gcols,
                                                      const double* __restrict__ lb, double* __restrict__ lsum) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < n_cols; ++c) {
        if (cover[c] >= 0) continue;
        const double v = vals[(size_t)c * n + i];
        if (v != v) continue;
        double term = lb[(size_t)c * n + i];
        if (labels[c].mode == DENSE_LGMM) term += flog(v);
        s += term;
    }
    for (int g = 0; g < n_groups; ++g) {
        bool active = true;
        double jac = 0.0;
        for (int d = goff[g]; d < goff[g + 1]; ++d) {
            const double v = vals[(size_t)gcols[d] * n + i];
            active &= v == v;
            if (labels[gcols[d]].mode == DENSE_LGMM) jac += flog(v);
        }
        if (!active) continue;
        const double term = lb[(size_t)(n_cols + g) * n + i] + jac;
        s += term;
    }
    lsum[i] = s;
}

// One round's keys: entry i's standard Gumbel noise from its own Philox
// counter (i, 0, TPE_POOL_STREAM, round) -- 52 bits of the first two words,
// u = (t + 0.5) 2^-52 strictly inside (0, 1), G = -log(-log u) -- added to
// lsum[i].  The sort key is 0 for an entry that is not free; keys_out
// (diagnostics) gets every entry's key.
__global__ __launch_bounds__(kBlock) void k_pool_key(const double* __restrict__ lsum,
                                                     const uint8_t* __restrict__ taken, int64_t n, uint32_t k0,
                                                     uint32_t k1, uint32_t round, uint64_t* __restrict__ key,
                                                     uint32_t* __restrict__ idx, double* __restrict__ keys_out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const U4 w = philox4x32_10(U4{(uint32_t)i, 0u, (uint32_t)TPE_POOL_STREAM, round}, k0, k1);
    const uint64_t t = ((uint64_t)w.x << 20) | (uint64_t)(w.y >> 12);
    const double u = ((double)t + 0.5) * 0x1.0p-52;
    const double gumbel = -flog(-flog(u));
    const double k = lsum[i] + gumbel;
    key[i] = taken[i] ? 0ull : order_key(k);
    idx[i] = (uint32_t)i;
    if (keys_out) keys_out[i] = k;
}

// the better of the workgroup's (key, index) pairs, in thread 0
__device__ __forceinline__ void pool_block_best(uint64_t& k, int64_t& i) {
    __shared__ uint64_t sk[kBlock / 64];
    __shared__ int64_t si[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ok = __shfl_down(k, off, 64);
        const int64_t oi = __shfl_down(i, off, 64);
        if (better(ok, oi, k, i)) {
            k = ok;
            i = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        sk[threadIdx.x >> 6] = k;
        si[threadIdx.x >> 6] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / 64; ++w)
            if (better(sk[w], si[w], k, i)) {
                k = sk[w];
                i = si[w];
            }
}

constexpr int64_t kNoEntry = INT64_MAX;   // with key 0 (no score's key): loses to every entry

// the best score among the first d sorted entries (the drawn set): a partial
// per workgroup, then one workgroup over the partials
__global__ __launch_bounds__(kBlock) void k_pool_pick(const uint32_t* __restrict__ idx,
                                                      const double* __restrict__ score, int64_t d,
                                                      uint64_t* __restrict__ part_k, int64_t* __restrict__ part_i) {
    uint64_t k = 0ull;
    int64_t i = kNoEntry;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < d; p += (int64_t)gridDim.x * kBlock) {
        const int64_t e = idx[p];
        const uint64_t ke = order_key(score[e]);
        if (better(ke, e, k, i)) {
            k = ke;
            i = e;
        }
    }
    pool_block_best(k, i);
    if (threadIdx.x == 0) {
        part_k[blockIdx.x] = k;
        part_i[blockIdx.x] = i;
    }
}

__global__ __launch_bounds__(kBlock) void k_pool_pick_final(const uint64_t* __restrict__ part_k,
                                                            const int64_t* __restrict__ part_i, int32_t n_part,
                                                            const double* __restrict__ score, int64_t n,
                                                            int64_t* __restrict__ best_i,
                                                            double* __restrict__ best_s) {
    uint64_t k = 0ull;
    int64_t i = kNoEntry;
    for (int p = threadIdx.x; p < n_part; p += kBlock)
        if (better(part_k[p], part_i[p], k, i)) {
            k = part_k[p];
            i = part_i[p];
        }
    pool_block_best(k, i);
    if (threadIdx.x == 0) {
        *best_i = i;
        *best_s = (i >= 0 && i < n) ? score[i] : __builtin_nan("");
    }
}

__global__ __launch_bounds__(kBlock) void k_pool_drawn(const uint32_t* __restrict__ idx, int64_t d,
                                                       int64_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p < d) out[p] = (int64_t)idx[p];
}

__global__ void k_pool_take(const int64_t* __restrict__ best_i, int64_t n, uint8_t* __restrict__ flag) {
    const int64_t i = *best_i;
    if (i >= 0 && i < n) flag[i] = 1;
}

struct PoolState {
    int64_t n = 0;
    int32_t n_cols = 0;
    DevBuf<double> vals;                 // [n_cols][n]
    DevBuf<double> lb, la;               // [n_cols + n_groups][n]
    DevBuf<double> score, gvals, top_s;
    DevBuf<uint64_t> key, key2;
    DevBuf<uint32_t> idx, idx2;
    DevBuf<uint8_t> taken, tmp;
    DevBuf<int64_t> taken_i, top_i;
    DevBuf<int32_t> meta;                // cover [n_cols] | goff [n_groups + 1] | gcols
    // the columns with at most kPoolUniq distinct values (found by tpe_pool_set
    // on the host): their values, concatenated; per column the offset of its
    // list (-1: none), its length and its slot in umap -- ucol = uoff | ucnt |
    // uslot, n_cols each; umap[slot][n]: each entry's position in the list
    // (0 for a NaN); ut_lb / ut_la: the lpdfs per listed value
    DevBuf<double> uvals, ut_lb, ut_la;
    DevBuf<int32_t> ucol;
    DevBuf<uint16_t> umap;
    // tpe_pool_draw: lsum [n]; the pick's partials; the diagnostics' vectors
    DevBuf<double> lsum, keys_all;
    DevBuf<uint64_t> part_k;
    DevBuf<int64_t> part_i, drawn;
    DevBuf<int32_t> err;
    PinVec<int32_t> err_h;
    PinVec<int64_t> top_i_h;
    PinVec<double> top_s_h;
};

PoolState* pool_of(tpe_ctx* ctx, bool make) {
    if (!ctx->pool && make)
        ctx->pool = std::shared_ptr<void>(new PoolState(), [](void* q) { delete static_cast<PoolState*>(q); });
    return static_cast<PoolState*>(ctx->pool.get());
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int tpe1_pool_set(tpe_ctx* ctx, const double* values, int64_t n, int32_t n_cols) {
    if (!ctx) return TPE_ERR_ARG;
    if (!values) return ctx->fail(TPE_ERR_ARG, "tpe_pool_set: null pointer");
    if (n < 1 || n_cols < 1) return ctx->fail(TPE_ERR_ARG, "tpe_pool_set: n and n_cols must be at least 1");
    if (n >= ((int64_t)1 << 31)) return ctx->fail(TPE_ERR_ARG, "tpe_pool_set: at most 2^31 - 1 entries");
    // column-major on the host (the one-time cost of a pool), rows in blocks
    // so that both sides stay in cache
    std::vector<double> t((size_t)n * n_cols);
    constexpr int64_t kRows = 256;
    for (int64_t r0 = 0; r0 < n; r0 += kRows) {
        const int64_t r1 = std::min(n, r0 + kRows);
        for (int64_t r = r0; r < r1; ++r)
            for (int32_t c = 0; c < n_cols; ++c) {
                const double v = values[(size_t)r * n_cols + c];
                if (std::isinf(v))
                    return ctx->fail(TPE_ERR_VALUE, "tpe_pool_set: entry " + std::to_string(r) + ", column " +
                                                        std::to_string(c) + " is infinite");
                t[(size_t)c * n + r] = v;
            }
    }
    // the columns on a grid: their distinct values by bit pattern (-0 as +0),
    // given up at the first value past kPoolUniq (a dense column: after about
    // that many entries)
    std::vector<int32_t> ucol(3 * (size_t)n_cols, -1);
    std::vector<double> uvals;
    std::vector<uint16_t> umap;
    {
        std::unordered_map<uint64_t, uint16_t> seen;
        std::vector<uint16_t> pos((size_t)n);
        std::vector<double> list;
        int32_t slots = 0;
        for (int32_t c = 0; c < n_cols; ++c) {
            seen.clear();
            list.clear();
            const double* col = t.data() + (size_t)c * n;
            bool few = true;
            for (int64_t r = 0; r < n && few; ++r) {
                double v = col[r];
                pos[r] = 0;
                if (v != v) continue;
                if (v == 0.0) v = 0.0;
                uint64_t b;
                std::memcpy(&b, &v, 8);
                auto it = seen.find(b);
                if (it == seen.end()) {
                    if (list.size() == kPoolUniq) {
                        few = false;
                        break;
                    }
                    it = seen.emplace(b, (uint16_t)list.size()).first;
                    list.push_back(v);
                }
                pos[r] = it->second;
            }
            if (!few || list.empty()) continue;
            ucol[c] = (int32_t)uvals.size();
            ucol[(size_t)n_cols + c] = (int32_t)list.size();
            ucol[2 * (size_t)n_cols + c] = slots++;
            uvals.insert(uvals.end(), list.begin(), list.end());
            umap.insert(umap.end(), pos.begin(), pos.end());
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    PoolState* S = pool_of(ctx, true);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (a ranking still reading the old pool)
    S->n = 0;
    S->n_cols = 0;
    HIPCHK(ctx, S->vals.reserve(t.size()));
    HIPCHK(ctx, hipMemcpy(S->vals.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, S->ucol.reserve(ucol.size()));
    HIPCHK(ctx, hipMemcpy(S->ucol.p, ucol.data(), ucol.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(ctx, S->uvals.reserve(std::max<size_t>(uvals.size(), 1)));
    HIPCHK(ctx, S->ut_lb.reserve(std::max<size_t>(uvals.size(), 1)));
    HIPCHK(ctx, S->ut_la.reserve(std::max<size_t>(uvals.size(), 1)));
    HIPCHK(ctx, S->umap.reserve(std::max<size_t>(umap.size(), 1)));
    if (!uvals.empty()) {
        HIPCHK(ctx, hipMemcpy(S->uvals.p, uvals.data(), uvals.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(S->umap.p, umap.data(), umap.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    S->n = n;
    S->n_cols = n_cols;
    return TPE_OK;
}

int tpe1_pool_clear(tpe_ctx* ctx) {
    if (!ctx) return TPE_ERR_ARG;
    if (ctx->pool) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->pool.reset();
    }
    return TPE_OK;
}

int tpe1_pool_size(const tpe_ctx* ctx, int64_t* n, int32_t* n_cols) {
    if (!ctx) return TPE_ERR_ARG;
    const PoolState* S = static_cast<const PoolState*>(ctx->pool.get());
    if (n) *n = S ? S->n : 0;
    if (n_cols) *n_cols = S ? S->n_cols : 0;
    return TPE_OK;
}

}  // extern "C"

namespace {

// What tpe_pool_rank and tpe_pool_draw share, `fn` naming the entry point in
// the messages: the checks of the context (pool_context) and of the groups and
// `taken` (pool_groups), then everything queued up to the scores (pool_scores).
struct PoolCall {
    PoolState* S = nullptr;
    int64_t n = 0;
    int32_t L = 0, n_groups = 0;
    std::vector<int32_t> meta;       // cover [L] | goff [n_groups + 1] | gcols
    int64_t n_free = 0;              // the entries not in `taken`
    size_t sort_bytes = 0;
    const int32_t* goff() const { return meta.data() + L; }
    const int32_t* d_cover() const { return S->meta.p; }
    const int32_t* d_goff() const { return S->meta.p + L; }
    const int32_t* d_gcols() const { return S->meta.p + L + n_groups + 1; }
};

int pool_context(tpe_ctx* ctx, const std::string& fn, PoolCall& pc) {
    TPE_SETTLE(ctx);
    if (!ctx->peers.empty()) return ctx->fail(TPE_ERR_ARG, fn + ": not available on a multi-device context");
    if (ctx->precision != TPE_F64) return ctx->fail(TPE_ERR_ARG, fn + ": needs a TPE_F64 context");
    PoolState* S = pool_of(ctx, false);
    if (!S || S->n < 1) return ctx->fail(TPE_ERR_ARG, fn + ": no pool set (tpe_pool_set)");
    Posterior& P = ctx->resident;
    if (P.n_labels == 0) return ctx->fail(TPE_ERR_ARG, fn + ": no posterior set");
    if (S->n_cols != P.n_labels)
        return ctx->fail(TPE_ERR_ARG, fn + ": the pool has " + std::to_string(S->n_cols) +
                                          " columns, the posterior " + std::to_string(P.n_labels) + " labels");
    pc.S = S;
    pc.n = S->n;
    pc.L = S->n_cols;
    return TPE_OK;
}

int pool_groups(tpe_ctx* ctx, const std::string& fn, PoolCall& pc, int32_t n_groups, const int32_t* slots,
                const int64_t* group_off, const int32_t* group_cols, const int64_t* taken, int64_t n_taken) {
    if (n_groups < 0 || n_taken < 0 || (n_taken > 0 && !taken) ||
        (n_groups > 0 && (!slots || !group_off || !group_cols)))
        return ctx->fail(TPE_ERR_ARG, fn + ": null pointer or negative count");
    if (n_groups > TPE_JOINT_MAX_GROUPS) return ctx->fail(TPE_ERR_ARG, fn + ": too many groups");
    const int64_t n = pc.n;
    const int32_t L = pc.L;
    pc.n_groups = n_groups;
    // the groups: set, distinct slots; columns in range, in one group at most; D columns each
    const int64_t n_gc = n_groups ? group_off[n_groups] : 0;
    if (n_gc < 0 || n_gc > L) return ctx->fail(TPE_ERR_ARG, fn + ": the groups list more columns than the pool has");
    pc.meta.assign((size_t)L + n_groups + 1 + n_gc, -1);
    int32_t* cover = pc.meta.data();
    int32_t* goff = pc.meta.data() + L;
    int32_t* gcols = goff + n_groups + 1;
    goff[0] = 0;
    {
        bool seen[TPE_JOINT_MAX_GROUPS] = {};
        if (n_groups && group_off[0] != 0) return ctx->fail(TPE_ERR_ARG, fn + ": group_off[0] must be 0");
        for (int32_t g = 0; g < n_groups; ++g) {
            const int32_t slot = slots[g];
            int32_t D = 0;
            if (slot < 0 || slot >= TPE_JOINT_MAX_GROUPS || tpe1_joint_set_slots(ctx, slot, &D) != 1)
                return ctx->fail(TPE_ERR_ARG, fn + ": group " + std::to_string(g) + ": slot not set");
            if (seen[slot]) return ctx->fail(TPE_ERR_ARG, fn + ": slot " + std::to_string(slot) + " listed twice");
            seen[slot] = true;
            const int64_t a = group_off[g], b = group_off[g + 1];
            if (b < a || b - a != D)
                return ctx->fail(TPE_ERR_ARG, fn + ": group " + std::to_string(g) + " lists " +
                                                  std::to_string(b - a) + " columns, its slot has " +
                                                  std::to_string(D) + " dimensions");
            for (int64_t k = a; k < b; ++k) {
                const int32_t c = group_cols[k];
                if (c < 0 || c >= L)
                    return ctx->fail(TPE_ERR_ARG, fn + ": column " + std::to_string(c) + " out of range");
                if (cover[c] >= 0)
                    return ctx->fail(TPE_ERR_ARG, fn + ": column " + std::to_string(c) + " in two groups");
                cover[c] = g;
                gcols[k] = c;
            }
            goff[g + 1] = (int32_t)b;
        }
    }
    // the entries left after `taken` (duplicates and indices outside the pool ignored)
    pc.n_free = n;
    {
        std::vector<int64_t> tk;
        tk.reserve((size_t)n_taken);
        for (int64_t t = 0; t < n_taken; ++t)
            if (taken[t] >= 0 && taken[t] < n) tk.push_back(taken[t]);
        std::sort(tk.begin(), tk.end());
        pc.n_free -= (int64_t)(std::unique(tk.begin(), tk.end()) - tk.begin());
    }
    return TPE_OK;
}

// the call's planes, scores and rank keys, queued on the context's stream
// (n_out: the pairs the caller reads back); a joint group's error has
// synchronised the stream
int pool_scores(tpe_ctx* ctx, PoolCall& pc, const int32_t* slots, const int64_t* taken, int64_t n_taken,
                int64_t n_out) {
    PoolState* S = pc.S;
    Posterior& P = ctx->resident;
    const int64_t n = pc.n;
    const int32_t L = pc.L, n_groups = pc.n_groups;
    const std::vector<int32_t>& meta = pc.meta;
    const int32_t* goff = pc.goff();
    const int64_t n_top = n_out;
    size_t& sort_bytes = pc.sort_bytes;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t planes = (size_t)(L + n_groups) * n;
    HIPCHK(ctx, S->lb.reserve(planes));
    HIPCHK(ctx, S->la.reserve(planes));
    HIPCHK(ctx, S->score.reserve(n));
    HIPCHK(ctx, S->key.reserve(n));
    HIPCHK(ctx, S->key2.reserve(n));
    HIPCHK(ctx, S->idx.reserve(n));
    HIPCHK(ctx, S->idx2.reserve(n));
    HIPCHK(ctx, S->taken.reserve(n));
    HIPCHK(ctx, S->taken_i.reserve(std::max<int64_t>(n_taken, 1)));
    HIPCHK(ctx, S->meta.reserve(meta.size()));
    HIPCHK(ctx, S->err.reserve(1));
    HIPCHK(ctx, S->top_i.reserve(std::max<int64_t>(n_top, 1)));
    HIPCHK(ctx, S->top_s.reserve(std::max<int64_t>(n_top, 1)));
    HIPCHK(ctx, S->err_h.resize(1));
    HIPCHK(ctx, S->top_i_h.resize(std::max<int64_t>(n_top, 1)));
    HIPCHK(ctx, S->top_s_h.resize(std::max<int64_t>(n_top, 1)));
    hipcub::DoubleBuffer<uint64_t> kb(S->key.p, S->key2.p);
    hipcub::DoubleBuffer<uint32_t> vb(S->idx.p, S->idx2.p);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(nullptr, sort_bytes, kb, vb, (int)n, 0, 64, st));
    HIPCHK(ctx, S->tmp.reserve(std::max<size_t>(sort_bytes, 1)));
    size_t gv = 0;
    for (int32_t g = 0; g < n_groups; ++g) gv = std::max(gv, (size_t)(goff[g + 1] - goff[g]) * n);
    if (gv) HIPCHK(ctx, S->gvals.reserve(gv));

    HIPCHK(ctx, hipMemcpyAsync(S->meta.p, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(S->err.p, 0, sizeof(int32_t), st));
    HIPCHK(ctx, hipMemsetAsync(S->taken.p, 0, n, st));
    if (n_taken > 0) {
        HIPCHK(ctx, hipMemcpyAsync(S->taken_i.p, taken, n_taken * sizeof(int64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pool_mark, dim3(blocks_of(n_taken, kBlock)), dim3(kBlock), 0, st, S->taken_i.p, n_taken,
                           n, S->taken.p);
    }
    const int32_t* d_cover = S->meta.p;
    const int32_t* d_goff = S->meta.p + L;
    const int32_t* d_gcols = d_goff + n_groups + 1;
    // the per-label planes, one launch per family over the posterior's label lists
    const int32_t n_dense = (int32_t)(P.h_group[DENSE_GMM].size() + P.h_group[DENSE_LGMM].size());
    static_assert(DENSE_GMM == 0 && DENSE_LGMM == 1, "the dense families' lists are adjacent");
    if (n_dense)
        hipLaunchKernelGGL(k_pool_dense, dim3(blocks_of(n, kPoolTile), n_dense), dim3(kBlock), 0, st, P.labels.p,
                           P.groups.p + P.group_off[DENSE_GMM], P.comps64.p, S->vals.p, n, d_cover, S->lb.p,
                           S->la.p);
    const int32_t* d_uoff = S->ucol.p;
    const int32_t* d_ucnt = S->ucol.p + L;
    const int32_t* d_uslot = S->ucol.p + 2 * (size_t)L;
    for (int m : {QUANT_GMM, QUANT_LGMM}) {
        const int32_t nl = (int32_t)P.h_group[m].size();
        if (!nl) continue;
        const int32_t* grp = P.groups.p + P.group_off[m];
        const dim3 grid(blocks_of(n, kBlock), nl);
        if (m == QUANT_GMM)
            hipLaunchKernelGGL(k_pool_quant<QUANT_GMM>, grid, dim3(kBlock), 0, st, P.labels.p, grp, P.comps64.p,
                               S->vals.p, n, d_cover, d_uoff, d_ucnt, S->uvals.p, S->ut_lb.p, S->ut_la.p, S->lb.p,
                               S->la.p, S->err.p);
        else
            hipLaunchKernelGGL(k_pool_quant<QUANT_LGMM>, grid, dim3(kBlock), 0, st, P.labels.p, grp, P.comps64.p,
                               S->vals.p, n, d_cover, d_uoff, d_ucnt, S->uvals.p, S->ut_lb.p, S->ut_la.p, S->lb.p,
                               S->la.p, S->err.p);
        hipLaunchKernelGGL(k_pool_spread, grid, dim3(kBlock), 0, st, grp, S->vals.p, n, d_cover, d_uoff, d_uslot,
                           S->umap.p, S->ut_lb.p, S->ut_la.p, S->lb.p, S->la.p);
    }
    if (const int32_t nl = (int32_t)P.h_group[CAT].size())
        hipLaunchKernelGGL(k_pool_cat, dim3(blocks_of(n, kBlock), nl), dim3(kBlock), 0, st, P.labels.p,
                           P.groups.p + P.group_off[CAT], P.comps64.p, S->vals.p, n, d_cover, S->lb.p, S->la.p,
                           S->err.p);
    HIPCHK(ctx, hipGetLastError());
    // the groups' planes: gather, the joint score kernels, copy
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t D = goff[g + 1] - goff[g];
        hipLaunchKernelGGL(k_pool_gather, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, P.labels.p, S->vals.p, n,
                           d_gcols + goff[g], D, S->gvals.p);
        HIPCHK(ctx, hipGetLastError());
        double *ll = nullptr, *lg = nullptr;
        const int rc = tpe1_joint_score_device(ctx, slots[g], S->gvals.p, n, &ll, &lg);
        if (rc) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
        hipLaunchKernelGGL(k_pool_group, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, S->vals.p, n,
                           d_gcols + goff[g], D, ll, lg, S->lb.p + (size_t)(L + g) * n,
                           S->la.p + (size_t)(L + g) * n);
        HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_pool_sum, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, S->vals.p, n, L, d_cover,
                       n_groups, d_goff, d_gcols, S->lb.p, S->la.p, S->taken.p, S->score.p, S->key.p, S->idx.p);
    HIPCHK(ctx, hipGetLastError());
    return TPE_OK;
}

// after the call's synchronisation: what the kernels flagged in the values
int pool_flags(tpe_ctx* ctx, const std::string& fn, const PoolCall& pc) {
    const int32_t e = pc.S->err_h[0];
    if (e & 4) return ctx->fail(TPE_ERR_VALUE, fn + ": categorical value out of range");
    if (e & 2) return ctx->fail(TPE_ERR_VALUE, fn + ": negative arg to lognormal_cdf");
    return TPE_OK;
}

}  // namespace

extern "C" {

int tpe1_pool_rank(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const int64_t* group_off,
                   const int32_t* group_cols, const int64_t* taken, int64_t n_taken, int32_t top_k,
                   int64_t* top_index, double* top_score, int32_t* n_top_out, double* score, double* lpdf_below,
                   double* lpdf_above) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_pool_rank";
    PoolCall pc;
    if (const int rc = pool_context(ctx, fn, pc)) return rc;
    if (top_k < 1) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: top_k must be at least 1");
    if (!top_index || !top_score || !n_top_out || (lpdf_below == nullptr) != (lpdf_above == nullptr))
        return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: null pointer or negative count");
    if (const int rc = pool_groups(ctx, fn, pc, n_groups, slots, group_off, group_cols, taken, n_taken)) return rc;
    PoolState* S = pc.S;
    const int64_t n = pc.n;
    const int32_t L = pc.L;
    const int32_t n_top = (int32_t)std::min<int64_t>(top_k, pc.n_free);
    if (const int rc = pool_scores(ctx, pc, slots, taken, n_taken, n_top)) return rc;
    hipStream_t st = ctx->stream;
    const size_t planes = (size_t)(L + n_groups) * n;
    if (n_top > 0) {
        hipcub::DoubleBuffer<uint64_t> kb(S->key.p, S->key2.p);
        hipcub::DoubleBuffer<uint32_t> vb(S->idx.p, S->idx2.p);
        size_t sort_bytes = pc.sort_bytes;
        // stable and descending: equal keys keep their ascending index
        HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(S->tmp.p, sort_bytes, kb, vb, (int)n, 0, 64, st));
        hipLaunchKernelGGL(k_pool_top, dim3(blocks_of(n_top, kBlock)), dim3(kBlock), 0, st, vb.Current(), S->score.p,
                           n_top, S->top_i.p, S->top_s.p);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(S->top_i_h.data(), S->top_i.p, n_top * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   st));
        HIPCHK(ctx, hipMemcpyAsync(S->top_s_h.data(), S->top_s.p, n_top * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(S->err_h.data(), S->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    if (const int rc = pool_flags(ctx, fn, pc)) return rc;
    // the optional vectors (diagnostics) are plain copies after it: the
    // outputs stay untouched when the values were refused
    if (score) HIPCHK(ctx, hipMemcpy(score, S->score.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (lpdf_below) {
        // planes [L + n_groups][n] -> the caller's [n][L + n_groups]
        const int32_t W = L + n_groups;
        std::vector<double> h(planes);
        for (int side = 0; side < 2; ++side) {
            HIPCHK(ctx, hipMemcpy(h.data(), side ? S->la.p : S->lb.p, planes * sizeof(double),
                                  hipMemcpyDeviceToHost));
            double* dst = side ? lpdf_above : lpdf_below;
            for (int32_t c = 0; c < W; ++c)
                for (int64_t i = 0; i < n; ++i) dst[(size_t)i * W + c] = h[(size_t)c * n + i];
        }
    }
    std::memcpy(top_index, S->top_i_h.data(), (size_t)n_top * sizeof(int64_t));
    std::memcpy(top_score, S->top_s_h.data(), (size_t)n_top * sizeof(double));
    *n_top_out = n_top;
    return TPE_OK;
}

int tpe1_pool_draw(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const int64_t* group_off,
                   const int32_t* group_cols, const int64_t* taken, int64_t n_taken, uint64_t seed,
                   const uint32_t* rounds, int32_t n_rounds, int64_t m, int32_t distinct, int64_t* best_index,
                   double* best_score, int32_t* n_best_out, int64_t* drawn, int32_t* n_drawn, double* lsum,
                   double* keys, double* score) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_pool_draw";
    PoolCall pc;
    if (const int rc = pool_context(ctx, fn, pc)) return rc;
    if (m < 1) return ctx->fail(TPE_ERR_ARG, "tpe_pool_draw: m must be at least 1");
    if (n_rounds < 1 || n_rounds > 4096) return ctx->fail(TPE_ERR_ARG, "tpe_pool_draw: n_rounds must be in [1, 4096]");
    if (!rounds || !best_index || !best_score || !n_best_out || (drawn == nullptr) != (n_drawn == nullptr))
        return ctx->fail(TPE_ERR_ARG, "tpe_pool_draw: null pointer or negative count");
    if (const int rc = pool_groups(ctx, fn, pc, n_groups, slots, group_off, group_cols, taken, n_taken)) return rc;
    PoolState* S = pc.S;
    const int64_t n = pc.n;
    // what is free is known here round by round: the rounds that find an
    // entry, and how many each draws
    const int64_t cap = std::min(m, n);
    const int32_t n_best = distinct ? (int32_t)std::min<int64_t>(n_rounds, pc.n_free) : (pc.n_free > 0 ? n_rounds : 0);
    const auto drawn_in = [&](int32_t j) { return std::min(m, pc.n_free - (distinct ? j : 0)); };
    if (const int rc = pool_scores(ctx, pc, slots, taken, n_taken, n_rounds)) return rc;
    hipStream_t st = ctx->stream;
    constexpr int kPickBlocks = 256;
    HIPCHK(ctx, S->lsum.reserve(n));
    HIPCHK(ctx, S->part_k.reserve(kPickBlocks));
    HIPCHK(ctx, S->part_i.reserve(kPickBlocks));
    if (keys) HIPCHK(ctx, S->keys_all.reserve((size_t)n_rounds * n));
    if (drawn) HIPCHK(ctx, S->drawn.reserve((size_t)n_rounds * cap));
    hipLaunchKernelGGL(k_pool_lsum, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, ctx->resident.labels.p, S->vals.p,
                       n, pc.L, pc.d_cover(), n_groups, pc.d_goff(), pc.d_gcols(), S->lb.p, S->lsum.p);
    HIPCHK(ctx, hipGetLastError());
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
    // `keys` asks for every round's keys, the rounds past the last pick included
    for (int32_t j = 0; j < (keys ? n_rounds : n_best); ++j) {
        hipLaunchKernelGGL(k_pool_key, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, S->lsum.p, S->taken.p, n, k0,
                           k1, rounds[j], S->key.p, S->idx.p, keys ? S->keys_all.p + (size_t)j * n : nullptr);
        HIPCHK(ctx, hipGetLastError());
        if (j >= n_best) continue;
        const int64_t d = drawn_in(j);
        // stable and descending: equal keys keep their ascending index, and
        // the entries that are not free (key 0) come last
        hipcub::DoubleBuffer<uint64_t> kb(S->key.p, S->key2.p);
        hipcub::DoubleBuffer<uint32_t> vb(S->idx.p, S->idx2.p);
        HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairsDescending(S->tmp.p, pc.sort_bytes, kb, vb, (int)n, 0, 64, st));
        const int32_t n_part = (int32_t)std::min<int64_t>(blocks_of(d, kBlock), kPickBlocks);
        hipLaunchKernelGGL(k_pool_pick, dim3(n_part), dim3(kBlock), 0, st, vb.Current(), S->score.p, d, S->part_k.p,
                           S->part_i.p);
        hipLaunchKernelGGL(k_pool_pick_final, dim3(1), dim3(kBlock), 0, st, S->part_k.p, S->part_i.p, n_part,
                           S->score.p, n, S->top_i.p + j, S->top_s.p + j);
        if (drawn)
            hipLaunchKernelGGL(k_pool_drawn, dim3(blocks_of(d, kBlock)), dim3(kBlock), 0, st, vb.Current(), d,
                               S->drawn.p + (size_t)j * cap);
        if (distinct) hipLaunchKernelGGL(k_pool_take, dim3(1), dim3(1), 0, st, S->top_i.p + j, n, S->taken.p);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_best > 0) {
        HIPCHK(ctx, hipMemcpyAsync(S->top_i_h.data(), S->top_i.p, n_best * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   st));
        HIPCHK(ctx, hipMemcpyAsync(S->top_s_h.data(), S->top_s.p, n_best * sizeof(double), hipMemcpyDeviceToHost,
                                   st));
    }
    HIPCHK(ctx, hipMemcpyAsync(S->err_h.data(), S->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    if (const int rc = pool_flags(ctx, fn, pc)) return rc;
    // the optional vectors (diagnostics), copied after it as in tpe_pool_rank
    if (score) HIPCHK(ctx, hipMemcpy(score, S->score.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (lsum) HIPCHK(ctx, hipMemcpy(lsum, S->lsum.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (keys) HIPCHK(ctx, hipMemcpy(keys, S->keys_all.p, (size_t)n_rounds * n * sizeof(double), hipMemcpyDeviceToHost));
    if (drawn) {
        for (int32_t j = 0; j < n_best; ++j)
            HIPCHK(ctx, hipMemcpy(drawn + (size_t)j * cap, S->drawn.p + (size_t)j * cap,
                                  (size_t)drawn_in(j) * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int32_t j = 0; j < n_rounds; ++j) n_drawn[j] = j < n_best ? (int32_t)drawn_in(j) : 0;
    }
    std::memcpy(best_index, S->top_i_h.data(), (size_t)n_best * sizeof(int64_t));
    std::memcpy(best_score, S->top_s_h.data(), (size_t)n_best * sizeof(double));
    *n_best_out = n_best;
    return TPE_OK;
}

}  // extern "C"
