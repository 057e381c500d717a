// tpe_cmodel.hip -- the constraint-density round (c-TPE): one objective model
// and up to eight constraint models per label, each a below / above pair of
// Parzen mixtures (include/hyperopt_tpe.h, tpe_cmodel_*; DESIGN.md section
// "Constraint densities").
//
// Model 0 is the context's resident posterior; model k >= 1 is a posterior
// uploaded by tpe_cmodel_set through the same fold as tpe_set_posterior.  Per
// label the non-skipped models M' (ascending) each contribute n candidates
// drawn from their below mixture, every candidate is scored under both sides
// of every model of M', and
//     a(x) = sum_k f(gamma_k, lg_k(x) - ll_k(x))
// picks the winner in broadcast_best's order.
//
// The shape is the opposite of the plain round's: few candidates per label
// (n |M'| <= a few hundred) against above mixtures of the order of the trial
// count, so the work is split over COMPONENTS:
//   k_cm_draw     one workgroup per (round, label): the n |M'| values
//   k_cm_partial  grid (chunk, model side, round x label): kCmChunk components
//                 of one mixture staged once in LDS as structure-of-arrays (a
//                 term's read is one broadcast), candidates in lanes, a
//                 one-pass online log-sum-exp (dense) or the linear interval
//                 mass (quantized) per lane; one (max, sum) per (candidate,
//                 chunk) at a fixed address -- no atomics
//   k_cm_finish   one workgroup per (round, label): the chunk partials merged
//                 in ascending chunk order, the lpdfs, t_k, f, a, the winner
// Every sum has a fixed order, so a and the winner are the same bits from run
// to run and do not depend on the grid.
//
// Layout in HBM (per context, grown on demand):
//   lab   : CmLabel[L]                 M', streams, gammas, chunk rows
//   cand  : double[cells][NC]          NC = n max|M'| (score: n)
//   part  : double2[rounds][rows][NC]  rows = the labels' chunk rows
//   res   : tpe_label_result[cells]
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

constexpr int kCmModels = 9;      // the objective and up to 8 constraints
constexpr int kCmSides = 2 * kCmModels;
constexpr int kCmChunk = 1024;    // components per workgroup of k_cm_partial
constexpr int kCmWaves = kBlock / 64;

// the models' device arrays (one record in device memory, read per workgroup)
struct CmPtrs {
    const DLabel* labels[kCmModels];
    const Comp<double>* comps[kCmModels];
    const SampRec* samp[kCmModels];
};

struct CmLabel {
    int32_t mode, nm;                 // the label's family; |M'|
    int32_t model[kCmModels];         // M', ascending
    uint32_t stream[kCmModels];       // the Philox stream of each model of M'
    int32_t chunk_off[kCmSides + 1];  // prefix of the chunk counts over s = 2 mi + side
    int32_t base;                     // the label's first row in a round's partial plane
    double gamma[kCmModels];          // by position in M'
};

// -log(gamma + (1 - gamma) e^t), evaluated on the side where the exponential
// cannot overflow; NaN t gives NaN, t = +inf gives -inf, t = -inf gives -log gamma
__device__ __forceinline__ double cm_f(double gamma, double t) {
#pragma clang fp contract(off)
    if (t <= 0.0) return -log(gamma + (1.0 - gamma) * exp(t));
    return -(t + log((1.0 - gamma) + gamma * exp(-t)));
}

// Candidate j = mi n + g of a cell: draw g of model M'[mi]'s below mixture with
// that model's stream -- the plain round's draw (sample_below), values only.
__global__ __launch_bounds__(kBlock) void k_cm_draw(const CmPtrs* __restrict__ Pp,
                                                    const CmLabel* __restrict__ lab, int32_t n_labels,
                                                    int32_t n, int32_t NC, uint64_t seed,
                                                    const uint32_t* __restrict__ rounds, double* __restrict__ cand,
                                                    int32_t* __restrict__ err) {
    const int32_t cell = blockIdx.x, l = cell % n_labels;
    const uint32_t round = rounds[cell / n_labels];
    const CmLabel& C = lab[l];
    const int32_t nc = n * C.nm;
    for (int32_t j = threadIdx.x; j < nc; j += kBlock) {
        const int32_t mi = j / n, k = C.model[mi];
        DLabel L = Pp->labels[k][l];
        L.stream = (int32_t)C.stream[mi];
        const SampRec* s = Pp->samp[k] + L.samp_off;
        const uint32_t g = (uint32_t)(j - mi * n);
        double v = 0.0;
        bool ok;
        switch (L.mode) {
            case DENSE_GMM: ok = sample_below<DENSE_GMM>(L, s, seed, round, g, v); break;
            case DENSE_LGMM: ok = sample_below<DENSE_LGMM>(L, s, seed, round, g, v); break;
            case QUANT_GMM: ok = sample_below<QUANT_GMM>(L, s, seed, round, g, v); break;
            case QUANT_LGMM: ok = sample_below<QUANT_LGMM>(L, s, seed, round, g, v); break;
            default: ok = sample_below<CAT>(L, s, seed, round, g, v); break;
        }
        if (!ok) atomicOr(err, 1);
        cand[(int64_t)cell * NC + j] = v;
    }
}

// One chunk of one mixture against every candidate of a cell.
//   dense: the records are tpe_set_posterior's (m', a', c' in exp_scaled units,
//     c' <= 0): u_k = c'_k - (x' a'_k - m'_k)^2, and the lane keeps the running
//     maximum M of u and S = sum_k exp((u_k - M) / K), rescaled only when M
//     moves -- one exp_scaled per term, no underflow wherever the candidate lies;
//   quantized: quant_lpdf's loop over the chunk (linear domain, no contraction).
// Categorical labels have no chunks (k_cm_finish reads their table).
// only_label >= 0: the probe's single cell of that label.
__global__ __launch_bounds__(kBlock) void k_cm_partial(const CmPtrs* __restrict__ Pp,
                                                       const CmLabel* __restrict__ lab, int32_t n_labels,
                                                       int32_t only_label, int32_t n_per, int32_t NC,
                                                       int64_t rows, const double* __restrict__ cand,
                                                       double2* __restrict__ part, int32_t* __restrict__ err) {
    const int32_t cell = blockIdx.z;
    const int32_t l = only_label >= 0 ? only_label : cell % n_labels;
    const int32_t z = only_label >= 0 ? 0 : cell / n_labels;
    const CmLabel& C = lab[l];
    const int32_t s = blockIdx.y, mi = s >> 1, side = s & 1;
    if (mi >= C.nm) return;   // (uniform over the workgroup, as the next)
    const int32_t c = blockIdx.x;
    if (c >= C.chunk_off[s + 1] - C.chunk_off[s]) return;
    const int32_t k = C.model[mi];
    const DLabel L = Pp->labels[k][l];
    const int32_t n_side = side ? L.na : L.nb;
    const Comp<double>* __restrict__ src = Pp->comps[k] + (side ? L.comp_a : L.comp_b) + (int64_t)c * kCmChunk;
    const int32_t cnt = min(kCmChunk, n_side - c * kCmChunk);
    const bool dense = L.mode == DENSE_GMM || L.mode == DENSE_LGMM;

    __shared__ double sm[kCmChunk], sa[kCmChunk], sc[kCmChunk];   // mu, a, c (dense) / w (quantized)
    __shared__ double exp_tab[kExpTabSize];
    for (int32_t i = threadIdx.x; i < cnt; i += kBlock) {
        const Comp<double> r = src[i];
        sm[i] = r.mu;
        sa[i] = r.a;
        sc[i] = dense ? r.c : r.w;
    }
    if (dense) load_exp_table(exp_tab);   // (ends with a barrier)
    else __syncthreads();

    const int32_t nc = only_label >= 0 ? n_per : n_per * C.nm;
    const int64_t row = (int64_t)z * rows + C.base + C.chunk_off[s] + c;
    const double ninf = -__builtin_inf();
    // (a wave whose candidates all lie past nc has nothing to do)
    for (int32_t j = threadIdx.x; j < nc; j += kBlock) {
        const double x = cand[(int64_t)cell * NC + j];
        double2 out;
        if (dense) {
            const double y = L.mode == DENSE_LGMM ? flog(x) : x;
            const double xr = y - L.centre;
            double M = ninf, S = 0.0;
            for (int32_t i = 0; i < cnt; ++i) {
                const double zz = fma(xr, sa[i], -sm[i]);
                const double u = fma(-zz, zz, sc[i]);
                if (u > M) {   // the maximum moves: rescale what was summed
                    S = M == ninf ? 1.0 : fma(S, exp_scaled(M - u, exp_tab), 1.0);
                    M = u;
                } else if (!(u == ninf)) {   // (a NaN term makes the sum NaN)
                    S = exp_scaled_acc(u - M, exp_tab, S);
                }
            }
            out = double2{M, S};
        } else {
            double ub, lo;
            bool neg;
            if (L.mode == QUANT_LGMM) quant_bounds<QUANT_LGMM>(L, x, ub, lo, neg);
            else quant_bounds<QUANT_GMM>(L, x, ub, lo, neg);
            if (neg) atomicOr(err, 2);
            double prob = 0.0;
            {
#pragma clang fp contract(off)
                if (L.mode == QUANT_LGMM) {
                    for (int32_t i = 0; i < cnt; ++i) {
                        const double pu = 0.5 + 0.5 * erf((ub - sm[i]) * sa[i]);
                        const double pl = 0.5 + 0.5 * erf((lo - sm[i]) * sa[i]);
                        double inc = sc[i] * pu;
                        inc -= sc[i] * pl;
                        prob += inc;
                    }
                } else {
                    for (int32_t i = 0; i < cnt; ++i) {
                        const double pu = 0.5 * (1.0 + erf((ub - sm[i]) * sa[i]));
                        const double pl = 0.5 * (1.0 + erf((lo - sm[i]) * sa[i]));
                        double inc = sc[i] * pu;
                        inc -= sc[i] * pl;
                        prob += inc;
                    }
                }
            }
            out = double2{0.0, prob};
        }
        part[row * NC + j] = out;
    }
}

// one side's lpdf of candidate j from its chunk partials, ascending chunks
__device__ __forceinline__ double cm_side_lpdf(const DLabel& L, const Comp<double>* __restrict__ comps, int32_t side,
                                               double x, const double2* __restrict__ p, int32_t nchunks,
                                               int64_t stride) {
    if (L.mode == CAT) {
        int64_t s = (int64_t)x;
        s = s < 0 ? 0 : (s >= L.nb ? L.nb - 1 : s);
        return comps[(side ? L.comp_a : L.comp_b) + s].c;
    }
    if (L.mode == QUANT_GMM || L.mode == QUANT_LGMM) {
        double prob = 0.0;
        for (int32_t c = 0; c < nchunks; ++c) prob += p[c * stride].y;
        return flog(prob) - (side ? L.logpacc_a : L.logpacc_b);
    }
    const double ninf = -__builtin_inf();
    double M = ninf;
    for (int32_t c = 0; c < nchunks; ++c) M = fmax(M, p[c * stride].x);
    if (!(M > ninf)) return __builtin_nan("");   // no term at all: the reference's row maximum is -inf
    double S = 0.0;
    for (int32_t c = 0; c < nchunks; ++c) {
        const double2 q = p[c * stride];
        if (q.x > ninf) S += q.y * exp((q.x - M) * kExpScaleInv);
    }
    double v = log(S) + M * kExpScaleInv + (side ? L.shift_a : L.shift_b);
    if (L.mode == DENSE_LGMM) v -= flog(x);
    return v;
}

// Per cell: the lpdfs of every candidate under every model of M', a, and the
// winner (order_key / better: NaN greatest, lowest index on ties).  The probe
// (only_label >= 0) also writes a and the planes ll / lg [kCmModels][n].
__global__ __launch_bounds__(kBlock) void k_cm_finish(const CmPtrs* __restrict__ Pp,
                                                      const CmLabel* __restrict__ lab, int32_t n_labels,
                                                      int32_t only_label, int32_t n_per, int32_t NC, int64_t rows,
                                                      const double* __restrict__ cand,
                                                      const double2* __restrict__ part,
                                                      tpe_label_result* __restrict__ res, double* __restrict__ acq,
                                                      double* __restrict__ out_ll, double* __restrict__ out_lg) {
    const int32_t cell = blockIdx.x;
    const int32_t l = only_label >= 0 ? only_label : cell % n_labels;
    const int32_t z = only_label >= 0 ? 0 : cell / n_labels;
    const CmLabel& C = lab[l];
    const int32_t nc = only_label >= 0 ? n_per : n_per * C.nm;
    uint64_t bk = 0;
    int64_t bi = -1;
    double bv = 0.0, ba = 0.0, bll = 0.0, blg = 0.0;
    for (int32_t j = threadIdx.x; j < nc; j += kBlock) {
        const double x = cand[(int64_t)cell * NC + j];
        double a = 0.0, ll0 = 0.0, lg0 = 0.0;
        for (int32_t mi = 0; mi < C.nm; ++mi) {
            const int32_t k = C.model[mi];
            const DLabel L = Pp->labels[k][l];
            const Comp<double>* __restrict__ comps = Pp->comps[k];
            double lp[2];
#pragma unroll
            for (int32_t side = 0; side < 2; ++side) {
                const int32_t s = 2 * mi + side;
                const int64_t row = (int64_t)z * rows + C.base + C.chunk_off[s];
                lp[side] = cm_side_lpdf(L, comps, side, x, part + row * NC + j,
                                        C.chunk_off[s + 1] - C.chunk_off[s], NC);
            }
            a += cm_f(C.gamma[mi], lp[1] - lp[0]);
            if (mi == 0) {
                ll0 = lp[0];
                lg0 = lp[1];
            }
            if (out_ll) {
                out_ll[(int64_t)k * n_per + j] = lp[0];
                out_lg[(int64_t)k * n_per + j] = lp[1];
            }
        }
        if (acq) acq[j] = a;
        const uint64_t key = order_key(a);
        if (bi < 0 || better(key, j, bk, bi)) {
            bk = key;
            bi = j;
            bv = x;
            ba = a;
            bll = ll0;
            blg = lg0;
        }
    }
    // the workgroup's winner: a shuffle tree per wave, then the wave winners
    __shared__ uint64_t wk[kCmWaves];
    __shared__ int64_t wi[kCmWaves];
    __shared__ int64_t win;
    uint64_t k2 = bk;
    int64_t i2 = bi;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ok = __shfl_down(k2, off, 64);
        const int64_t oi = __shfl_down(i2, off, 64);
        if (oi >= 0 && (i2 < 0 || better(ok, oi, k2, i2))) {
            k2 = ok;
            i2 = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        wk[threadIdx.x >> 6] = k2;
        wi[threadIdx.x >> 6] = i2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t k3 = wk[0];
        int64_t i3 = wi[0];
        for (int w = 1; w < kCmWaves; ++w)
            if (wi[w] >= 0 && (i3 < 0 || better(wk[w], wi[w], k3, i3))) {
                k3 = wk[w];
                i3 = wi[w];
            }
        win = i3;
        if (i3 < 0) res[cell] = tpe_label_result{__builtin_nan(""), __builtin_nan(""), __builtin_nan(""),
                                                  __builtin_nan(""), -1, l, 0};
    }
    __syncthreads();
    if (bi >= 0 && bi == win) res[cell] = tpe_label_result{bv, ba, bll, blg, bi, l, 0};
}

struct CmState {
    Posterior post[kCmModels];            // [1 .. 8]: the uploaded constraint models
    bool set[kCmModels] = {};
    std::vector<uint8_t> skip[kCmModels];   // per label: the model has no mixture for it
    DevBuf<CmLabel> lab;
    PinVec<CmLabel> lab_h;
    DevBuf<CmPtrs> ptrs;
    PinVec<CmPtrs> ptrs_h;
    DevBuf<double> cand, acq, ll, lg;
    DevBuf<double2> part;
    DevBuf<uint32_t> rounds;
    DevBuf<int32_t> err;
    DevBuf<tpe_label_result> res;
    PinVec<tpe_label_result> res_h;
    PinVec<int32_t> err_h;
    PinVec<uint32_t> rounds_h;
    PinVec<double> cand_h, acq_h;
};

CmState* cm_of(tpe_ctx* ctx) {
    if (!ctx->cmodel)
        ctx->cmodel = std::shared_ptr<void>(new CmState(), [](void* q) { delete static_cast<CmState*>(q); });
    return static_cast<CmState*>(ctx->cmodel.get());
}

int mode_of(const tpe_label_desc& d) {
    const bool quant = (d.flags & TPE_HAS_Q) != 0;
    if (d.kind == TPE_CATEGORICAL) return CAT;
    if (d.kind == TPE_GMM1) return quant ? QUANT_GMM : DENSE_GMM;
    if (d.kind == TPE_LGMM1) return quant ? QUANT_LGMM : DENSE_LGMM;
    return -1;
}

// what every entry point needs of the context
int cm_check_ctx(tpe_ctx* ctx, const std::string& fn) {
    if (!ctx->peers.empty()) return ctx->fail(TPE_ERR_ARG, fn + ": not available on a multi-device context");
    if (ctx->precision != TPE_F64) return ctx->fail(TPE_ERR_ARG, fn + ": needs a TPE_F64 context");
    if (ctx->resident.n_labels == 0) return ctx->fail(TPE_ERR_ARG, fn + ": no posterior set");
    return TPE_OK;
}

// The labels' table for a call: M', streams, gammas (gammas[l * gstride + k])
// and the chunk rows.  *rows: chunk rows of one round; *max_nm, *max_chunks.
int cm_plan(tpe_ctx* ctx, CmState* S, const std::string& fn, const double* gammas, int32_t gstride,
            int32_t only_label, int64_t* rows, int32_t* max_nm, int32_t* max_chunks, const CmPtrs** ptrs) {
    Posterior& P = ctx->resident;
    const int32_t L = P.n_labels;
    for (int k = 1; k < kCmModels; ++k)
        if (S->set[k] && S->post[k].n_labels != L)
            return ctx->fail(TPE_ERR_ARG, fn + ": constraint model " + std::to_string(k) +
                                              " was set for another posterior (label count)");
    HIPCHK(ctx, S->lab_h.resize(L));
    int64_t r = 0;
    int32_t mnm = 1, mch = 0;
    for (int32_t l = 0; l < L; ++l) {
        const DLabel& d0 = P.h_labels[l];
        CmLabel C;
        std::memset(&C, 0, sizeof(C));
        C.mode = d0.mode;
        if ((uint32_t)d0.stream >= TPE_CMODEL_STREAM_SPAN)
            return ctx->fail(TPE_ERR_ARG, fn + ": a label's stream exceeds TPE_CMODEL_STREAM_SPAN");
        for (int k = 0; k < kCmModels; ++k) {
            if (k > 0 && (!S->set[k] || S->skip[k][l])) continue;
            if (k > 0 && S->post[k].h_labels[l].mode != d0.mode)
                return ctx->fail(TPE_ERR_ARG, fn + ": constraint model " + std::to_string(k) + ", label " +
                                                  std::to_string(l) + ": kind differs from the posterior's");
            const double g = gammas[(int64_t)(only_label >= 0 ? 0 : l) * gstride + k];
            if ((only_label < 0 || l == only_label) && !(g > 0.0 && g <= 1.0))
                return ctx->fail(TPE_ERR_ARG, fn + ": gamma of model " + std::to_string(k) + " must lie in (0, 1]");
            const int mi = C.nm++;
            C.model[mi] = k;
            C.stream[mi] = k == 0 ? (uint32_t)d0.stream
                                  : TPE_CMODEL_STREAM + (uint32_t)(k - 1) * TPE_CMODEL_STREAM_SPAN + (uint32_t)d0.stream;
            C.gamma[mi] = g;
        }
        const bool planned = only_label < 0 || l == only_label;   // (the probe plans its label's rows alone)
        C.base = (int32_t)r;
        for (int mi = 0; mi < kCmModels; ++mi)
            for (int side = 0; side < 2; ++side) {
                int32_t nch = 0;
                if (planned && mi < C.nm && d0.mode != CAT) {
                    const DLabel& d = C.model[mi] == 0 ? d0 : S->post[C.model[mi]].h_labels[l];
                    nch = ((side ? d.na : d.nb) + kCmChunk - 1) / kCmChunk;
                }
                C.chunk_off[2 * mi + side + 1] = C.chunk_off[2 * mi + side] + nch;
                if (only_label < 0 || l == only_label) mch = std::max(mch, nch);
            }
        r += C.chunk_off[kCmSides];
        if (r > (int64_t)1 << 30) return ctx->fail(TPE_ERR_ARG, fn + ": too many components");
        if (only_label < 0 || l == only_label) mnm = std::max(mnm, C.nm);
        S->lab_h[l] = C;
    }
    *rows = std::max<int64_t>(r, 1);
    *max_nm = mnm;
    *max_chunks = mch;
    HIPCHK(ctx, S->ptrs_h.resize(1));
    HIPCHK(ctx, S->ptrs.reserve(1));
    for (int k = 0; k < kCmModels; ++k) {
        Posterior& Q = k == 0 ? P : S->post[k];
        const bool on = k == 0 || S->set[k];
        S->ptrs_h[0].labels[k] = on ? Q.labels.p : nullptr;
        S->ptrs_h[0].comps[k] = on ? Q.comps64.p : nullptr;
        S->ptrs_h[0].samp[k] = on ? Q.samp.p : nullptr;
    }
    HIPCHK(ctx, hipMemcpyAsync(S->ptrs.p, S->ptrs_h.data(), sizeof(CmPtrs), hipMemcpyHostToDevice, ctx->stream));
    *ptrs = S->ptrs.p;
    HIPCHK(ctx, S->lab.reserve(L));
    HIPCHK(ctx, hipMemcpyAsync(S->lab.p, S->lab_h.data(), (size_t)L * sizeof(CmLabel), hipMemcpyHostToDevice,
                               ctx->stream));
    return TPE_OK;
}

int cm_err(tpe_ctx* ctx, int32_t e) {
    if (e & 1) return ctx->fail(TPE_ERR_SAMPLE, "truncated sampler: interval [low, high) not reached");
    if (e & 2) return ctx->fail(TPE_ERR_VALUE, "negative arg to lognormal_cdf");
    return TPE_OK;
}

}  // namespace

extern "C" {

int tpe_cmodel_set(tpe_ctx* ctx, int32_t k, const tpe_label_desc* labels, int32_t n_labels, const double* weights,
                   const double* mus, const double* sigmas, int64_t n_components) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_cmodel_set";
    TPE_SETTLE(ctx);
    if (int rc = cm_check_ctx(ctx, fn)) return rc;
    if (k < 1 || k >= kCmModels) return ctx->fail(TPE_ERR_ARG, fn + ": k must lie in [1, 8]");
    Posterior& P = ctx->resident;
    if (!labels || n_labels != P.n_labels)
        return ctx->fail(TPE_ERR_ARG, fn + ": the label count must be the posterior's");
    if (n_components < 0 || (n_components > 0 && !weights)) return ctx->fail(TPE_ERR_ARG, fn + ": null pointer");
    CmState* S = cm_of(ctx);
    // a label without components on a side is skipped for k: the fold still
    // needs a mixture for it, so it gets a placeholder that no kernel reads
    std::vector<tpe_label_desc> d(labels, labels + n_labels);
    std::vector<double> w(weights, weights + n_components), m((size_t)n_components, 0.0),
        s((size_t)n_components, 1.0);
    if (mus) m.assign(mus, mus + n_components);
    if (sigmas) s.assign(sigmas, sigmas + n_components);
    std::vector<uint8_t> skip((size_t)n_labels, 0);
    for (int32_t l = 0; l < n_labels; ++l) {
        const DLabel& d0 = P.h_labels[l];
        if (mode_of(d[l]) != d0.mode)
            return ctx->fail(TPE_ERR_ARG, fn + ": label " + std::to_string(l) + ": kind differs from the posterior's");
        if (d[l].n_below < 0 || d[l].n_above < 0) return ctx->fail(TPE_ERR_ARG, fn + ": negative component count");
        if (d[l].n_below > 0 && d[l].n_above > 0) continue;
        skip[l] = 1;
        const int32_t cnt = d0.mode == CAT ? d0.nb : 1;
        const bool bounded = (d[l].flags & 3) == 3;
        d[l].below_off = d[l].above_off = (int64_t)w.size();
        d[l].n_below = d[l].n_above = cnt;
        for (int32_t i = 0; i < cnt; ++i) {
            w.push_back(1.0 / cnt);
            m.push_back(bounded ? 0.5 * d[l].low + 0.5 * d[l].high : 0.0);
            s.push_back(1.0);
        }
    }
    S->set[k] = false;
    ctx->P = &S->post[k];
    const int rc = tpe1_set_posterior(ctx, d.data(), n_labels, w.data(), m.data(), s.data(), (int64_t)w.size());
    ctx->P = &ctx->resident;
    if (rc) return rc;
    S->skip[k] = skip;
    S->set[k] = true;
    return TPE_OK;
}

int tpe_cmodel_clear(tpe_ctx* ctx) {
    if (!ctx) return TPE_ERR_ARG;
    if (!ctx->cmodel) return TPE_OK;
    CmState* S = static_cast<CmState*>(ctx->cmodel.get());
    for (int k = 0; k < kCmModels; ++k) S->set[k] = false;   // (the buffers are kept for the next models)
    return TPE_OK;
}

int tpe_cmodel_score(tpe_ctx* ctx, int32_t label, const double* cand, int64_t n, const double* gammas,
                     double* acq_out, double* ll_out, double* lg_out) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_cmodel_score";
    TPE_SETTLE(ctx);
    if (int rc = cm_check_ctx(ctx, fn)) return rc;
    Posterior& P = ctx->resident;
    if (label < 0 || label >= P.n_labels) return ctx->fail(TPE_ERR_ARG, fn + ": label out of range");
    if (n < 1 || n > (1 << 20) || !cand || !gammas || !acq_out || (ll_out == nullptr) != (lg_out == nullptr))
        return ctx->fail(TPE_ERR_ARG, fn + ": null pointer or n outside [1, 2^20]");
    // what the reference raises before computing, as tpe_score checks it
    const DLabel& d = P.h_labels[label];
    if (d.mode == QUANT_LGMM)
        for (int64_t i = 0; i < n; ++i) {
            double ub = cand[i] + d.q / 2.0;
            if ((d.flags & 2) && ub > d.exp_high) ub = d.exp_high;
            if (ub < 0) return ctx->fail(TPE_ERR_VALUE, fn + ": negative arg to lognormal_cdf");
        }
    if (d.mode == CAT)
        for (int64_t i = 0; i < n; ++i)
            if (!(cand[i] >= 0 && cand[i] < d.nb) || cand[i] != std::floor(cand[i]))
                return ctx->fail(TPE_ERR_VALUE, fn + ": categorical sample out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CmState* S = cm_of(ctx);
    int64_t rows;
    int32_t max_nm, max_chunks;
    const CmPtrs* ptrs;
    if (int rc = cm_plan(ctx, S, fn, gammas, kCmModels, label, &rows, &max_nm, &max_chunks, &ptrs)) return rc;
    const int32_t NC = (int32_t)n;
    HIPCHK(ctx, S->cand.reserve(n));
    HIPCHK(ctx, S->acq.reserve(n));
    HIPCHK(ctx, S->part.reserve((size_t)rows * NC));
    HIPCHK(ctx, S->res.reserve(1));
    HIPCHK(ctx, S->err.reserve(1));
    HIPCHK(ctx, S->err_h.resize(1));
    HIPCHK(ctx, S->cand_h.resize(n));
    HIPCHK(ctx, S->acq_h.resize(n));
    if (ll_out) {
        HIPCHK(ctx, S->ll.reserve((size_t)kCmModels * n));
        HIPCHK(ctx, S->lg.reserve((size_t)kCmModels * n));
    }
    std::memcpy(S->cand_h.data(), cand, (size_t)n * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(S->cand.p, S->cand_h.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(S->err.p, 0, sizeof(int32_t), st));
    if (ll_out) {   // (all-ones bytes are a NaN: the rows of the skipped models)
        HIPCHK(ctx, hipMemsetAsync(S->ll.p, 0xFF, (size_t)kCmModels * n * sizeof(double), st));
        HIPCHK(ctx, hipMemsetAsync(S->lg.p, 0xFF, (size_t)kCmModels * n * sizeof(double), st));
    }
    if (max_chunks > 0)
        hipLaunchKernelGGL(k_cm_partial, dim3((unsigned)max_chunks, 2u * (unsigned)max_nm, 1u), dim3(kBlock), 0, st,
                           ptrs, S->lab.p, P.n_labels, label, NC, NC, rows, S->cand.p, S->part.p, S->err.p);
    hipLaunchKernelGGL(k_cm_finish, dim3(1), dim3(kBlock), 0, st, ptrs, S->lab.p, P.n_labels, label, NC, NC, rows,
                       S->cand.p, S->part.p, S->res.p, S->acq.p, ll_out ? S->ll.p : nullptr,
                       ll_out ? S->lg.p : nullptr);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(S->acq_h.data(), S->acq.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(S->err_h.data(), S->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    if (int rc = cm_err(ctx, S->err_h[0])) return rc;
    std::memcpy(acq_out, S->acq_h.data(), (size_t)n * sizeof(double));
    if (ll_out) {   // the planes are plain copies after it
        HIPCHK(ctx, hipMemcpy(ll_out, S->ll.p, (size_t)kCmModels * n * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(lg_out, S->lg.p, (size_t)kCmModels * n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return TPE_OK;
}

int tpe_cmodel_suggest_batch(tpe_ctx* ctx, uint64_t seed, const uint32_t* rounds, int32_t n_rounds,
                             int64_t n_candidates, const double* gammas, tpe_label_result* results) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_cmodel_suggest_batch";
    TPE_SETTLE(ctx);
    if (int rc = cm_check_ctx(ctx, fn)) return rc;
    Posterior& P = ctx->resident;
    const int32_t L = P.n_labels;
    if (!rounds || !gammas || !results || n_rounds < 1 || n_candidates < 1 || n_candidates > (1 << 16))
        return ctx->fail(TPE_ERR_ARG, fn + ": null pointer, no round, or n_candidates outside [1, 2^16]");
    const int64_t cells = (int64_t)n_rounds * L;
    if (cells > 65535) return ctx->fail(TPE_ERR_ARG, fn + ": more than 65535 (round, label) cells");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CmState* S = cm_of(ctx);
    int64_t rows;
    int32_t max_nm, max_chunks;
    const CmPtrs* ptrs;
    if (int rc = cm_plan(ctx, S, fn, gammas, kCmModels, -1, &rows, &max_nm, &max_chunks, &ptrs)) return rc;
    const int32_t n = (int32_t)n_candidates, NC = n * max_nm;
    HIPCHK(ctx, S->cand.reserve((size_t)cells * NC));
    HIPCHK(ctx, S->part.reserve((size_t)n_rounds * rows * NC));
    HIPCHK(ctx, S->res.reserve(cells));
    HIPCHK(ctx, S->rounds.reserve(n_rounds));
    HIPCHK(ctx, S->err.reserve(1));
    HIPCHK(ctx, S->err_h.resize(1));
    HIPCHK(ctx, S->res_h.resize(cells));
    HIPCHK(ctx, S->rounds_h.resize(n_rounds));
    std::memcpy(S->rounds_h.data(), rounds, (size_t)n_rounds * sizeof(uint32_t));
    HIPCHK(ctx, hipMemcpyAsync(S->rounds.p, S->rounds_h.data(), (size_t)n_rounds * sizeof(uint32_t),
                               hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(S->err.p, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_cm_draw, dim3((unsigned)cells), dim3(kBlock), 0, st, ptrs, S->lab.p, L, n, NC, seed,
                       S->rounds.p, S->cand.p, S->err.p);
    if (max_chunks > 0)
        hipLaunchKernelGGL(k_cm_partial, dim3((unsigned)max_chunks, 2u * (unsigned)max_nm, (unsigned)cells),
                           dim3(kBlock), 0, st, ptrs, S->lab.p, L, -1, n, NC, rows, S->cand.p, S->part.p, S->err.p);
    hipLaunchKernelGGL(k_cm_finish, dim3((unsigned)cells), dim3(kBlock), 0, st, ptrs, S->lab.p, L, -1, n, NC, rows,
                       S->cand.p, S->part.p, S->res.p, (double*)nullptr, (double*)nullptr, (double*)nullptr);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(S->res_h.data(), S->res.p, (size_t)cells * sizeof(tpe_label_result),
                               hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(S->err_h.data(), S->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    if (int rc = cm_err(ctx, S->err_h[0])) return rc;
    std::memcpy(results, S->res_h.data(), (size_t)cells * sizeof(tpe_label_result));
    return TPE_OK;
}

}  // extern "C"
