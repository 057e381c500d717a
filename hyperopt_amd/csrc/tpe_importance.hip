// tpe_importance.hip -- hyperparameter importance from the resident Parzen
// mixtures (include/hyperopt_tpe.h, tpe_importance; DESIGN.md section 6b,
// "Hyperparameter importance").
//
// Per selected label d, with alpha_d the share of its observations among the
// good trials, l_d / g_d its below / above mixture and cells (x_j, w_j):
//   p(x) = alpha l(x) + (1 - alpha) g(x)       the density of its observed values
//   m(x) = alpha l(x) / p(x)                   P(good | x_d = x)
//   V_d  = sum_j w_j p(x_j) (m(x_j) - alpha)^2
// The lpdfs are the ones tpe_score returns (lse_dense, quant_bounds /
// quant_lpdf, the categorical log p table); a cell of a quantized label that
// merges `merge` support values takes the quantized lpdf with the step
// merge q.
//
// Layout in HBM (per context, grown on demand):
//   x, w   : double[N]        the cells of the selected labels, concatenated
//   lb, la : double[N]        the lpdf planes (written only when asked for)
//   part   : double[G]        one partial per (label, granule of kBlock cells)
//   v      : double[n_sel]
// Kernels, one launch per family over (cell tiles, labels of the family):
//   k_imp_dense   lse_dense on both mixtures + the term + the granule sums
//   k_imp_quant   quant_bounds / quant_lpdf      (GMM1 and LGMM1 instances)
//   k_imp_cat     the log p table
//   k_imp_sum     per label: its partials added in ascending granule order
// Every sum has a fixed order -- lanes by a shuffle tree, waves and granules
// ascending -- and a partial belongs to one label's granule whatever the tile
// or the other labels of the call, so v is the same bits from run to run,
// alone or among others.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"
#include "tpe_device.h"

using namespace tpe;
using namespace tpe_rt;

namespace {

// Cells per thread of the dense kernel: a tile is kImpR granules.  At 32
// labels x 4096 cells a tile of 512 cells gives 256 workgroups, one per CU;
// lse_dense sums a lane's components in the same order for every R, and the
// partials are per granule, so neither the lpdfs nor v depend on it.
constexpr int kImpR = 2;
constexpr int kImpWaves = kBlock / 64;

struct ImpSel {
    int32_t label, merge;
    int64_t off, n;      // the label's cells: [off, off + n) of x / w
    int64_t part;        // its first partial
    double alpha;
};

// w p (m - alpha)^2 from the two lpdfs, without cancellation: with d = lb - la
// and t = e^d - 1, m - alpha = alpha (1 - alpha) t / (1 + alpha t); for d > 0
// the same through t = e^-d - 1.  A cell neither mixture reaches (-inf, -inf)
// contributes 0; a NaN lpdf gives NaN.
__device__ __forceinline__ double imp_term(double lb, double la, double w, double alpha) {
#pragma clang fp contract(off)
    const double ninf = -__builtin_inf();
    if (lb == ninf && la == ninf) return 0.0;
    const double om = 1.0 - alpha;
    const double d = lb - la;
    double dev;
    if (d <= 0.0) {
        const double t = expm1(d);
        dev = alpha * om * t / (1.0 + alpha * t);
    } else {
        const double t = expm1(-d);
        dev = -(alpha * om * t) / (1.0 + om * t);
    }
    const double p = alpha * exp(lb) + om * exp(la);
    return w * p * (dev * dev);
}

// the lanes' terms of one granule, summed in a fixed order: a shuffle tree
// inside each wave, the wave sums ascending (thread 0 holds the result after
// the caller's barrier; `ws` one row of kImpWaves doubles per granule)
__device__ __forceinline__ void imp_wave_sums(double term, double* __restrict__ ws) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) term += __shfl_down(term, off, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = term;
}

__device__ __forceinline__ double imp_granule_sum(const double* __restrict__ ws) {
    double s = ws[0];
#pragma unroll
    for (int k = 1; k < kImpWaves; ++k) s += ws[k];
    return s;
}

// Dense GMM1 / LGMM1 labels: grid (cell tiles, selected dense labels), the
// factor of k_pool_dense (k_round<double, DENSE_*, false>'s) on the cells.
template <int R>
__global__ __launch_bounds__(kBlock) void k_imp_dense(const DLabel* __restrict__ labels,
                                                      const Comp<double>* __restrict__ comps,
                                                      const ImpSel* __restrict__ sel,
                                                      const int32_t* __restrict__ fam,
                                                      const double* __restrict__ xs, const double* __restrict__ wts,
                                                      double* __restrict__ part, double* __restrict__ out_lb,
                                                      double* __restrict__ out_la) {
    const ImpSel S = sel[fam[blockIdx.y]];
    const int64_t i0 = (int64_t)blockIdx.x * (kBlock * R);
    if (i0 >= S.n) return;   // (uniform over the workgroup)
    const DLabel L = labels[S.label];
    __shared__ double exp_tab[kExpTabSize];
    __shared__ double ws[R][kImpWaves];
    load_exp_table(exp_tab);
    const bool lgmm = L.mode == DENSE_LGMM;
    double y[R], lb[R], la[R];
    bool in[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = i0 + r * kBlock + threadIdx.x;
        in[r] = i < S.n;
        // (a lane past the label's cells scores a harmless value, as the pool's idle lanes do)
        const double x = in[r] ? xs[S.off + i] : (lgmm ? 1.0 : 0.0);
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
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = i0 + r * kBlock + threadIdx.x;
        double term = 0.0;
        if (in[r]) {
            term = imp_term(lb[r], la[r], wts[S.off + i], S.alpha);
            if (out_lb) {
                out_lb[S.off + i] = lb[r];
                out_la[S.off + i] = la[r];
            }
        }
        imp_wave_sums(term, ws[r]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (i0 + r * kBlock < S.n) part[S.part + (int64_t)blockIdx.x * R + r] = imp_granule_sum(ws[r]);
    }
}

// Quantized labels: grid (granules, selected labels of the family); the
// interval of a cell is quant_bounds' with the step merge q.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_imp_quant(const DLabel* __restrict__ labels,
                                                      const Comp<double>* __restrict__ comps64,
                                                      const ImpSel* __restrict__ sel,
                                                      const int32_t* __restrict__ fam,
                                                      const double* __restrict__ xs, const double* __restrict__ wts,
                                                      double* __restrict__ part, double* __restrict__ out_lb,
                                                      double* __restrict__ out_la) {
    const ImpSel S = sel[fam[blockIdx.y]];
    const int64_t i0 = (int64_t)blockIdx.x * kBlock;
    if (i0 >= S.n) return;
    DLabel L = labels[S.label];
    L.q = (double)S.merge * L.q;
    __shared__ double ws[kImpWaves];
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < S.n;
    double term = 0.0;
    // A wave whose lanes all lie past the label's cells skips the walk over
    // the components (wave-uniform: the wave's first cell); its terms are 0
    // either way.  The idle lanes of a partly filled wave walk along on a
    // harmless value -- they cost their wave nothing.
    if (i0 + (threadIdx.x & ~63) < S.n) {
        const double x = in ? xs[S.off + i] : (MODE == QUANT_LGMM ? 1.0 : 0.0);
        double ub, lo;
        bool neg;
        quant_bounds<MODE>(L, x, ub, lo, neg);   // (a negative upper end was refused on the host)
        const double lb = quant_lpdf<MODE == QUANT_LGMM>(comps64 + L.comp_b, L.nb, ub, lo, L.logpacc_b);
        const double la = quant_lpdf<MODE == QUANT_LGMM>(comps64 + L.comp_a, L.na, ub, lo, L.logpacc_a);
        if (in) {
            term = imp_term(lb, la, wts[S.off + i], S.alpha);
            if (out_lb) {
                out_lb[S.off + i] = lb;
                out_la[S.off + i] = la;
            }
        }
    }
    imp_wave_sums(term, ws);
    __syncthreads();
    if (threadIdx.x == 0) part[S.part + blockIdx.x] = imp_granule_sum(ws);
}

// Categorical labels: log p of the cell's category (checked on the host)
__global__ __launch_bounds__(kBlock) void k_imp_cat(const DLabel* __restrict__ labels,
                                                    const Comp<double>* __restrict__ comps64,
                                                    const ImpSel* __restrict__ sel, const int32_t* __restrict__ fam,
                                                    const double* __restrict__ xs, const double* __restrict__ wts,
                                                    double* __restrict__ part, double* __restrict__ out_lb,
                                                    double* __restrict__ out_la) {
    const ImpSel S = sel[fam[blockIdx.y]];
    const int64_t i0 = (int64_t)blockIdx.x * kBlock;
    if (i0 >= S.n) return;
    const DLabel L = labels[S.label];
    __shared__ double ws[kImpWaves];
    const int64_t i = i0 + threadIdx.x;
    double term = 0.0;
    if (i < S.n) {
        int64_t s = (int64_t)xs[S.off + i];
        s = s < 0 ? 0 : (s >= L.nb ? L.nb - 1 : s);
        const double lb = comps64[L.comp_b + s].c, la = comps64[L.comp_a + s].c;
        term = imp_term(lb, la, wts[S.off + i], S.alpha);
        if (out_lb) {
            out_lb[S.off + i] = lb;
            out_la[S.off + i] = la;
        }
    }
    imp_wave_sums(term, ws);
    __syncthreads();
    if (threadIdx.x == 0) part[S.part + blockIdx.x] = imp_granule_sum(ws);
}

// v[s]: from 0.0, the label's partials in ascending granule order
__global__ __launch_bounds__(kBlock) void k_imp_sum(const ImpSel* __restrict__ sel, int32_t n_sel,
                                                    const double* __restrict__ part, double* __restrict__ v) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_sel) return;
    const ImpSel S = sel[s];
    const int64_t ng = (S.n + kBlock - 1) / kBlock;
    double sum = 0.0;
    for (int64_t g = 0; g < ng; ++g) sum += part[S.part + g];
    v[s] = sum;
}

struct ImpState {
    DevBuf<double> x, w, lb, la, part, v;
    DevBuf<ImpSel> sel;
    DevBuf<int32_t> fam;
    PinVec<double> v_h;
};

ImpState* imp_of(tpe_ctx* ctx) {
    if (!ctx->imp) ctx->imp = std::shared_ptr<void>(new ImpState(), [](void* q) { delete static_cast<ImpState*>(q); });
    return static_cast<ImpState*>(ctx->imp.get());
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int tpe_importance(tpe_ctx* ctx, int32_t n_sel, const int32_t* labels, const int64_t* cell_off, const double* x,
                   const double* w, const int32_t* merge, const double* alpha, double* v, double* lb, double* la) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_importance";
    TPE_NOT_LSHARD(ctx);
    TPE_SETTLE(ctx);
    if (ctx->precision != TPE_F64) return ctx->fail(TPE_ERR_ARG, fn + ": needs a TPE_F64 context");
    Posterior& P = ctx->resident;
    if (P.n_labels == 0) return ctx->fail(TPE_ERR_ARG, fn + ": no posterior set");
    if (n_sel < 0 || (n_sel > 0 && (!labels || !cell_off || !merge || !alpha || !v)) || (lb == nullptr) != (la == nullptr))
        return ctx->fail(TPE_ERR_ARG, fn + ": null pointer or negative count");
    if (n_sel == 0) return TPE_OK;
    if (cell_off[0] != 0) return ctx->fail(TPE_ERR_ARG, fn + ": cell_off[0] must be 0");
    const int64_t N = cell_off[n_sel];
    // the selection: each label once, its cells, its first partial; the
    // families' lists (selection positions) in the order of the launches
    std::vector<ImpSel> sel((size_t)n_sel);
    std::vector<int32_t> fam_of[kNumModes];
    std::vector<uint8_t> seen((size_t)P.n_labels, 0);
    int64_t n_part = 0, max_n[kNumModes] = {};
    for (int32_t s = 0; s < n_sel; ++s) {
        const std::string at = fn + ": selection " + std::to_string(s);
        const int32_t l = labels[s];
        if (l < 0 || l >= P.n_labels) return ctx->fail(TPE_ERR_ARG, at + ": label out of range");
        if (seen[l]) return ctx->fail(TPE_ERR_ARG, at + ": label " + std::to_string(l) + " listed twice");
        seen[l] = 1;
        if (!(alpha[s] > 0.0 && alpha[s] < 1.0)) return ctx->fail(TPE_ERR_ARG, at + ": alpha must lie in (0, 1)");
        const DLabel& d = P.h_labels[l];
        const bool quant = d.mode == QUANT_GMM || d.mode == QUANT_LGMM;
        if (merge[s] < 1 || (merge[s] != 1 && !quant))
            return ctx->fail(TPE_ERR_ARG, at + ": merge must be at least 1, and 1 for a label that is not quantized");
        const int64_t a = cell_off[s], b = cell_off[s + 1];
        if (b < a) return ctx->fail(TPE_ERR_ARG, at + ": cell_off decreases");
        if (b > a && (!x || !w)) return ctx->fail(TPE_ERR_ARG, fn + ": null pointer or negative count");
        // what the reference raises before computing, as tpe_score checks it
        if (d.mode == CAT) {
            for (int64_t i = a; i < b; ++i)
                if (!(x[i] >= 0 && x[i] < d.nb) || x[i] != std::floor(x[i]))
                    return ctx->fail(TPE_ERR_VALUE, fn + ": categorical point out of range");
        } else if (d.mode == QUANT_LGMM) {
            const double half = (double)merge[s] * d.q / 2.0;
            for (int64_t i = a; i < b; ++i) {
                double ub = x[i] + half;
                if ((d.flags & 2) && ub > d.exp_high) ub = d.exp_high;
                if (ub < 0) return ctx->fail(TPE_ERR_VALUE, fn + ": negative arg to lognormal_cdf");
            }
        }
        sel[s] = ImpSel{l, merge[s], a, b - a, n_part, alpha[s]};
        n_part += (b - a + kBlock - 1) / kBlock;
        if (b > a) {
            fam_of[d.mode].push_back(s);
            max_n[d.mode] = std::max(max_n[d.mode], b - a);
        }
    }
    std::vector<int32_t> fam;
    int32_t fam_off[kNumModes + 1] = {};
    for (int m = 0; m < kNumModes; ++m) {
        fam.insert(fam.end(), fam_of[m].begin(), fam_of[m].end());
        fam_off[m + 1] = (int32_t)fam.size();
    }

    // (a multi-device context: its primary device)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ImpState* I = imp_of(ctx);
    HIPCHK(ctx, I->x.reserve(std::max<int64_t>(N, 1)));
    HIPCHK(ctx, I->w.reserve(std::max<int64_t>(N, 1)));
    HIPCHK(ctx, I->part.reserve(std::max<int64_t>(n_part, 1)));
    HIPCHK(ctx, I->v.reserve(n_sel));
    HIPCHK(ctx, I->sel.reserve(n_sel));
    HIPCHK(ctx, I->fam.reserve(std::max<size_t>(fam.size(), 1)));
    HIPCHK(ctx, I->v_h.resize(n_sel));
    if (lb) {
        HIPCHK(ctx, I->lb.reserve(std::max<int64_t>(N, 1)));
        HIPCHK(ctx, I->la.reserve(std::max<int64_t>(N, 1)));
    }
    if (N > 0) {
        HIPCHK(ctx, hipMemcpyAsync(I->x.p, x, N * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(I->w.p, w, N * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(I->sel.p, sel.data(), sel.size() * sizeof(ImpSel), hipMemcpyHostToDevice, st));
    if (!fam.empty())
        HIPCHK(ctx, hipMemcpyAsync(I->fam.p, fam.data(), fam.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    double* d_lb = lb ? I->lb.p : nullptr;
    double* d_la = lb ? I->la.p : nullptr;
    static_assert(DENSE_GMM == 0 && DENSE_LGMM == 1, "the dense families' lists are adjacent");
    if (const int32_t nl = fam_off[DENSE_LGMM + 1] - fam_off[DENSE_GMM])
        hipLaunchKernelGGL(k_imp_dense<kImpR>,
                           dim3(blocks_of(std::max(max_n[DENSE_GMM], max_n[DENSE_LGMM]), kBlock * kImpR), nl),
                           dim3(kBlock), 0, st, P.labels.p, P.comps64.p, I->sel.p, I->fam.p + fam_off[DENSE_GMM],
                           I->x.p, I->w.p, I->part.p, d_lb, d_la);
    if (const int32_t nl = fam_off[QUANT_GMM + 1] - fam_off[QUANT_GMM])
        hipLaunchKernelGGL(k_imp_quant<QUANT_GMM>, dim3(blocks_of(max_n[QUANT_GMM], kBlock), nl), dim3(kBlock), 0, st,
                           P.labels.p, P.comps64.p, I->sel.p, I->fam.p + fam_off[QUANT_GMM], I->x.p, I->w.p,
                           I->part.p, d_lb, d_la);
    if (const int32_t nl = fam_off[QUANT_LGMM + 1] - fam_off[QUANT_LGMM])
        hipLaunchKernelGGL(k_imp_quant<QUANT_LGMM>, dim3(blocks_of(max_n[QUANT_LGMM], kBlock), nl), dim3(kBlock), 0,
                           st, P.labels.p, P.comps64.p, I->sel.p, I->fam.p + fam_off[QUANT_LGMM], I->x.p, I->w.p,
                           I->part.p, d_lb, d_la);
    if (const int32_t nl = fam_off[CAT + 1] - fam_off[CAT])
        hipLaunchKernelGGL(k_imp_cat, dim3(blocks_of(max_n[CAT], kBlock), nl), dim3(kBlock), 0, st, P.labels.p,
                           P.comps64.p, I->sel.p, I->fam.p + fam_off[CAT], I->x.p, I->w.p, I->part.p, d_lb, d_la);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_imp_sum, dim3(blocks_of(n_sel, kBlock)), dim3(kBlock), 0, st, I->sel.p, n_sel, I->part.p,
                       I->v.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(I->v_h.data(), I->v.p, n_sel * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    std::memcpy(v, I->v_h.data(), (size_t)n_sel * sizeof(double));
    // the planes (asked for by the tests and the partial-dependence view) are plain copies after it
    if (lb && N > 0) {
        HIPCHK(ctx, hipMemcpy(lb, I->lb.p, N * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(la, I->la.p, N * sizeof(double), hipMemcpyDeviceToHost));
    }
    return TPE_OK;
}

}  // extern "C"
