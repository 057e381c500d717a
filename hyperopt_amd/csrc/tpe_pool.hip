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

int tpe1_pool_rank(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const int64_t* group_off,
                   const int32_t* group_cols, const int64_t* taken, int64_t n_taken, int32_t top_k,
                   int64_t* top_index, double* top_score, int32_t* n_top_out, double* score, double* lpdf_below,
                   double* lpdf_above) {
    if (!ctx) return TPE_ERR_ARG;
    TPE_SETTLE(ctx);
    if (!ctx->peers.empty())
        return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: not available on a multi-device context");
    if (ctx->precision != TPE_F64) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: needs a TPE_F64 context");
    PoolState* S = pool_of(ctx, false);
    if (!S || S->n < 1) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: no pool set (tpe_pool_set)");
    Posterior& P = ctx->resident;
    if (P.n_labels == 0) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: no posterior set");
    if (S->n_cols != P.n_labels)
        return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: the pool has " + std::to_string(S->n_cols) +
                                          " columns, the posterior " + std::to_string(P.n_labels) + " labels");
    if (top_k < 1) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: top_k must be at least 1");
    if (!top_index || !top_score || !n_top_out || (lpdf_below == nullptr) != (lpdf_above == nullptr) ||
        n_groups < 0 || n_taken < 0 || (n_taken > 0 && !taken) ||
        (n_groups > 0 && (!slots || !group_off || !group_cols)))
        return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: null pointer or negative count");
    if (n_groups > TPE_JOINT_MAX_GROUPS) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: too many groups");
    const int64_t n = S->n;
    const int32_t L = S->n_cols;
    // the groups: set, distinct slots; columns in range, in one group at most; D columns each
    const int64_t n_gc = n_groups ? group_off[n_groups] : 0;
    if (n_gc < 0 || n_gc > L) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: the groups list more columns than the pool has");
    std::vector<int32_t> meta((size_t)L + n_groups + 1 + n_gc, -1);
    int32_t* cover = meta.data();
    int32_t* goff = meta.data() + L;
    int32_t* gcols = goff + n_groups + 1;
    goff[0] = 0;
    {
        bool seen[TPE_JOINT_MAX_GROUPS] = {};
        if (n_groups && group_off[0] != 0) return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: group_off[0] must be 0");
        for (int32_t g = 0; g < n_groups; ++g) {
            const int32_t slot = slots[g];
            int32_t D = 0;
            if (slot < 0 || slot >= TPE_JOINT_MAX_GROUPS || tpe1_joint_set_slots(ctx, slot, &D) != 1)
                return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: group " + std::to_string(g) + ": slot not set");
            if (seen[slot])
                return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: slot " + std::to_string(slot) + " listed twice");
            seen[slot] = true;
            const int64_t a = group_off[g], b = group_off[g + 1];
            if (b < a || b - a != D)
                return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: group " + std::to_string(g) + " lists " +
                                                  std::to_string(b - a) + " columns, its slot has " +
                                                  std::to_string(D) + " dimensions");
            for (int64_t k = a; k < b; ++k) {
                const int32_t c = group_cols[k];
                if (c < 0 || c >= L)
                    return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: column " + std::to_string(c) + " out of range");
                if (cover[c] >= 0)
                    return ctx->fail(TPE_ERR_ARG, "tpe_pool_rank: column " + std::to_string(c) + " in two groups");
                cover[c] = g;
                gcols[k] = c;
            }
            goff[g + 1] = (int32_t)b;
        }
    }
    // the entries left after `taken` (duplicates and indices outside the pool ignored)
    int64_t n_free = n;
    {
        std::vector<int64_t> tk;
        tk.reserve((size_t)n_taken);
        for (int64_t t = 0; t < n_taken; ++t)
            if (taken[t] >= 0 && taken[t] < n) tk.push_back(taken[t]);
        std::sort(tk.begin(), tk.end());
        n_free -= (int64_t)(std::unique(tk.begin(), tk.end()) - tk.begin());
    }
    const int32_t n_top = (int32_t)std::min<int64_t>(top_k, n_free);

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
    HIPCHK(ctx, S->top_i.reserve(std::max(n_top, 1)));
    HIPCHK(ctx, S->top_s.reserve(std::max(n_top, 1)));
    HIPCHK(ctx, S->err_h.resize(1));
    HIPCHK(ctx, S->top_i_h.resize(std::max(n_top, 1)));
    HIPCHK(ctx, S->top_s_h.resize(std::max(n_top, 1)));
    size_t sort_bytes = 0;
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
    if (n_top > 0) {
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
    const int32_t e = S->err_h[0];
    if (e & 4) return ctx->fail(TPE_ERR_VALUE, "tpe_pool_rank: categorical value out of range");
    if (e & 2) return ctx->fail(TPE_ERR_VALUE, "tpe_pool_rank: negative arg to lognormal_cdf");
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

}  // extern "C"
