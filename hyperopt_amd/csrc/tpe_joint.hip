// tpe_joint.hip -- multivariate (joint) TPE: one product kernel per trial.
//
// The joint mixture of a side S has K = n_S + 1 components (0: the prior)
// over the D labels of the joint group, in each label's working space (log
// space for the log kinds):
//   f_S(y) = (1/A_S) sum_k W_k prod_d phi(y_d; mu_kd, s_kd)
//   A_S    = sum_k W_k prod_d m_kd,   m_kd the mass of N(mu_kd, s_kd) in [low_d, high_d)
//   lpdf_S = log f_S(y) - sum_{d log kind} y_d,   score = lpdf_below - lpdf_above
// Candidate g picks a below component with the pick word of the reserved
// stream TPE_JOINT_STREAM (thresholds ceil(cdf 2^32) of W_k prod_d m_kd) and
// draws every dimension from that component's normal truncated to the box
// with the label's own Philox words: icdf_draw on a one-component DrawComp.
//
// Kernels:
//   k_joint_fold / k_joint_fold_sum   records [k][d], masses, log A, thresholds
//   k_joint_round<DR, TABC, SAMPLE>   draw (or read) -> (max, sum) per slice of
//                                     kJSlice components -> merged in slice
//                                     order -> lpdfs -> per-workgroup best;
//                                     with few candidates one workgroup per
//                                     (tile, slice) stores the slice's pair and
//   k_joint_merge                     merges them, in the same order with the
//                                     same arithmetic: the same bits
//   k_joint_best                      the round's winner; its D values are
//                                     drawn again from Philox by index
//   k_joint_draw                      candidates and their components (tpe_joint_draw_group)
//   k_joint_best_cells                packed rounds (tpe_joint_suggest_batch): the
//                                     lanes of k_joint_round run over the flat
//                                     index f = r n + g of R rounds of n
//                                     candidates and store every candidate's
//                                     lpdfs; one workgroup per round slot r
//                                     reduces its n pairs and draws the winner
//   k_joint_gather<SCOTT>             tpe_joint_build_groups[_bw]: W, mu, sigma of every
//                                     group un-permuted out of the resident
//                                     univariate build (tpe_build.hip), one launch;
//                                     SCOTT (TPE_JOINT_BW_SCOTT): mu un-permuted the
//                                     same way, one sigma per (side, dimension) from
//                                     the host's factor; W is k_joint_weights'
//                                     (tpe_build.hip)
//   k_joint_interleave                that build under label shards: the slot's
//                                     [K][D] arrays from per-label columns
//   k_joint_cond_logw / _weights / _cols   tpe_joint_condition_group: a slot given some of
//                                     its dimensions -- L_k per component, each side's
//                                     log-sum-exp over one fixed tree and W'_k, the free
//                                     columns; then the fold above
//
// The extern "C" functions here are the per-device bodies tpe1_joint_*; the
// public tpe_joint_* names are tpe_multi.hip's, which replicates the groups
// over the devices of a multi-device context and shards the rounds.
//
// A context holds up to TPE_JOINT_MAX_GROUPS folded posteriors (slots), each
// with the Philox stream of its component pick; the scratch is shared.
//
// A posterior reaches a slot by one sequence, whoever supplies W / mu / sig:
// joint_layout (a group's checks, JDim records and categorical tables, from
// its per-dimension description), joint_reserve_slot, joint_upload_layout and
// the fill, joint_fold_group, one synchronisation, joint_commit.  The fill is the upload
// of joint_set (tpe_joint_set_group), the device-to-device copy of
// joint_condition (tpe_joint_condition_group), or the gather of a device build: one
// plan (JBuildPlan: joint_build_plan) and one driver (joint_build_gather, then
// joint_build_fold) for one device, for every device of a replicated context,
// and -- with a column buffer as the tasks' destination and the caller's
// barrier between the two -- for the devices of a label-sharded one.
//
// Arithmetic: component records are recentred and pre-scaled like the dense
// labels' (tpe_device.h, Comp): (m' = (mu - centre_d) a, a = sqrt(K/2)/s) with
// K = N/ln 2, so E_k = c_k - sum_d (y'_d a_kd - m'_kd)^2 is the exponent in
// exp_scaled's units; plain VALU FMAs, two per (candidate, component,
// dimension).  Records are wave-uniform; each lane holds one candidate, its
// y' in registers up to kJReg dimensions, beyond in LDS (dimension-major:
// consecutive lanes read consecutive words).
//
// Quantized dimensions (tpe_joint_set_group, q_d > 0): the mixtures, m_kd,
// A_S, the pick and the draw of y are the dense group's; the drawn value is
// x_d = rint(v / q_d) q_d (v = exp(y) for a log kind), and the factor of the
// dimension is the component's mass on the value's interval,
//   g_kd(x_d) = Phi((ub - mu_kd)/s_kd) - Phi((lb - mu_kd)/s_kd),   0 when ub <= lb,
// (ub, lb) = quant_bounds(x_d) in the working space (tpe_device.h).  No
// Jacobian term for a quantized log kind:
//   f_S(x) = (1/A_S) sum_k W_k prod_d g_kd(x_d)   (g = phi for dense d)
//   lpdf_S = log f_S(x) - sum_{d dense log kind} y_d
// Its record is (m' = (mu - centre_d) a, a = 1/(s sqrt 2)): z = bound' a - m',
// one FMA per interval end, and its -log(s sqrt(2 pi)) stays out of c_k.
// Accepted groups: S = D + (quantized dimensions) <= 128 values per candidate.
// A group with a quantized dimension runs k_joint_round<0, true, SAMPLE, true>:
// one wave per workgroup, the S values in LDS (512 S bytes; the exp table is
// read from memory) -- no register variant: the loop is bound by the VALU work
// of the two erfc-class evaluations per (candidate, component, quantized
// dimension), ~100 times the two LDS reads they share among kJU components.
// Dense-only groups launch the instantiations they always did.
//
// Categorical dimensions (tpe_joint_set_group, upper_d = C_d > 0, prior p_d):
// with a_Sd = C_d prior_weight / K_S the factor of category x in component k is
//   r_0d[x] = p_d[x],   r_td[x] = ([x == o_td] + a_Sd p_d[x]) / (1 + a_Sd)
// (o_td: the category trial t observed); m_kd = 1, so A_S and the pick are
// untouched, and there is no Jacobian term.  Evaluated as
//   log r_td[x] = log p_d[x] + log(a/(1+a)) + [x == o_td] log1p(1/(a p_d[o_td])):
// sum_d log p_d[x_d] rides with the candidate's ylog (subtracted), sum_d
// log(a/(1+a)) is in c_k of k >= 1, and the record is (o_kd, -K hit bonus),
// (-1, 0) for the prior component -- per (candidate, component, dimension) one
// compare, one select, one add on the candidate's category, its one LDS value.
// A value that is no integer in [0, C_d): factor 0, lpdf -inf on both sides.
// The draw takes word x of the Philox counter (g, 0, stream_d, round) and the
// first category c with ceil(cdf_kd[c] 2^32) above it, cdf_td[c] = (a P_d[c] +
// [c >= o_td]) / (a P_d[C-1] + 1) with P_d the running sums of p_d: a binary
// search over one table per dimension.  Such a group runs
// k_joint_round<0, true, SAMPLE, true, true>; groups without a categorical
// dimension launch the instantiations they always did.
#include "tpe_ctx.h"

#include <cmath>
#include <cstring>

namespace {
using namespace tpe;

constexpr int kJSlice = 32;        // components per (max, sum) slice
constexpr int kJU = 4;             // components sharing one read of y'_d
constexpr int kJReg = 32;          // dimensions a lane keeps in registers
constexpr int kJRegSmall = 8;
constexpr int kJLdsLanes = 64;     // workgroup of the LDS variant (one wave)
constexpr int kJLdsTabD = 64;      // up to here the exp table shares the LDS with y'
constexpr int kJMaxD = 128;
constexpr int kJBlock = 256;
constexpr int kJMaxBelow = 4096;
constexpr int kJMaxGroups = TPE_JOINT_MAX_GROUPS;
constexpr double kInf = __builtin_inf();

struct JDim {
    double low, high, centre;
    double q;          // the step of a quantized dimension, 0: dense
    double elo, ehi;   // exp(low), exp(high) of a bounded quantized log kind
    int32_t flags, stream, log;
    int32_t slot;      // quantized groups: the dimension's first per-candidate value
    int32_t upper;     // the categories of a categorical dimension, 0: not categorical
    int32_t cat_off;   // its first entry in the categorical tables
};

struct JDraw {   // one-component sampling terms of (k, d) (SampRec's);
    double mu, ssg, p0, q0, m;   // categorical: mu the observed category (-1: the prior), ssg = a_Sd
};

struct JP {   // the folded joint posterior
    const JDim* __restrict__ dims;
    const double2* __restrict__ rec;   // [k][d] (m', a); below components first
    const double* __restrict__ cst;    // [k] K (log W_k - sum_d log(s_kd sqrt(2 pi)))
    const double* __restrict__ logA;   // below, above
    const uint64_t* __restrict__ thr;  // [Kb] pick thresholds
    const JDraw* __restrict__ draw;    // [Kb][d]
    const double* __restrict__ catP;   // categorical tables at cat_off: running sums of p_d
    const double* __restrict__ catlp;  // log p_d
    int32_t D, Kb, Ka;
    uint32_t stream;                   // the pick word's Philox stream
};

__device__ __forceinline__ DLabel jlabel(const JDim& j) {
    DLabel L{};
    L.mode = j.log ? DENSE_LGMM : DENSE_GMM;
    L.flags = j.flags;
    L.low = j.low;
    L.high = j.high;
    L.stream = j.stream;
    return L;
}

// ------------------------------------------------------------------ fold ----
__global__ __launch_bounds__(kJBlock) void k_joint_fold(
    const JDim* __restrict__ dims, int32_t D, int32_t Kb, int32_t Ka, const double* __restrict__ W,
    const double* __restrict__ mu, const double* __restrict__ sig, double2* __restrict__ rec,
    double* __restrict__ cst, double* __restrict__ P, JDraw* __restrict__ draw, double pw,
    const double* __restrict__ catp) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * kJBlock + threadIdx.x;
    if (k >= Kb + Ka) return;
    double sl = 0.0, prod = 1.0;
    for (int d = 0; d < D; ++d) {
        const JDim j = dims[d];
        const size_t o = (size_t)k * D + d;
        if (j.upper > 0) {   // mass 1; mu holds the observed category (validated on the host)
            const bool prior = k == 0 || k == Kb;
            const double a = (double)j.upper * pw / (double)(k < Kb ? Kb : Ka);
            if (prior) {
                rec[o] = make_double2(-1.0, 0.0);
            } else {
                const double c = mu[o];
                rec[o] = make_double2(c, -(log1p(1.0 / (a * catp[j.cat_off + (int)c])) * kExpScale));
                sl += log1p(1.0 / a);   // -log(a / (1 + a))
            }
            if (k < Kb) draw[o] = JDraw{prior ? -1.0 : mu[o], a, 0.0, 0.0, 1.0};
            continue;
        }
        const double s = sig[o], m = mu[o];
        if (j.q > 0.0) {   // z = (bound - mu) / (s sqrt 2); its factor is a mass: no density constant
            const double a = 0.70710678118654752440 / s;
            rec[o] = make_double2((m - j.centre) * a, a);
        } else {
            const double a = sqrt(0.5 * kExpScale) / s;
            rec[o] = make_double2((m - j.centre) * a, a);
            sl += log(s * 2.50662827463100050242);
        }
        SampRec r{};
        r.mu = m;
        r.sigma = s;
        samp_trunc(jlabel(j), r);
        prod *= r.m;
        if (k < Kb) draw[o] = JDraw{r.mu, r.ssg, r.p0, r.q0, r.m};
    }
    cst[k] = (log(W[k]) - sl) * kExpScale;
    P[k] = W[k] * prod;
}

// block b: log A of side b (0 below, 1 above), by the same tree on both
// sides -- equal mixtures get equal log A; block 0 also the pick thresholds of
// the below side: its sum and cumulative weights in component order on one
// thread, as samp_fold_block forms them
__global__ __launch_bounds__(kJBlock) void k_joint_fold_sum(const double* __restrict__ P, int32_t Kb, int32_t Ka,
                                                            double* __restrict__ logA, uint64_t* __restrict__ thr,
                                                            int32_t* __restrict__ err) {
#pragma clang fp contract(off)
    const int side = blockIdx.x, K = side ? Ka : Kb;
    const double* Ps = P + (side ? Kb : 0);
    __shared__ double sh[kJBlock];
    double a = 0.0;
    for (int k = threadIdx.x; k < K; k += kJBlock) a += Ps[k];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int w = kJBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x) return;
    logA[side] = log(sh[0]);
    if (side) return;
    double Z = 0.0;
    for (int k = 0; k < Kb; ++k) Z += P[k];
    const bool zero = !(Z > 0.0);
    if (zero) atomicOr(err, 1);
    double run = 0.0;
    for (int k = 0; k < Kb; ++k) {
        run += P[k];
        thr[k] = pick_thr((k == Kb - 1 || zero) ? 1.0 : run / Z);
    }
}

// ------------------------------------------------------------------ draw ----
// the component of candidate g: the first k with thr[k] > wp of the group's pick stream
__device__ __forceinline__ int jpick(const JP& p, uint32_t k0, uint32_t k1, uint32_t g, uint32_t round) {
    DLabel L{};
    L.stream = (int32_t)p.stream;
    uint32_t wp, wu;
    draw_words(L, k0, k1, g, round, wp, wu);
    int lo = 0, hi = p.Kb - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.thr[mid] > (uint64_t)wp) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// categorical dimension d of candidate g from component k: the first category
// whose threshold ceil(cdf 2^32) is above word x of the counter (g, 0, stream,
// round) -- the independent round's categorical layout (sample_raw<CAT>); the
// last category's cdf is 1
__device__ __forceinline__ double jdraw_cat(const JP& p, const JDim& j, int d, int k, uint32_t k0, uint32_t k1,
                                            uint32_t g, uint32_t round) {
#pragma clang fp contract(off)
    const U4 w = philox4x32_10(U4{g, 0u, (uint32_t)j.stream, round}, k0, k1);
    const JDraw r = p.draw[(size_t)k * p.D + d];
    const double* __restrict__ P = p.catP + j.cat_off;
    const bool prior = r.mu < 0.0;
    const double Z = P[j.upper - 1], den = prior ? Z : r.ssg * Z + 1.0;
    int lo = 0, hi = j.upper - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double num = prior ? P[mid] : r.ssg * P[mid] + ((double)mid >= r.mu ? 1.0 : 0.0);
        if (pick_thr(num / den) > (uint64_t)w.x) hi = mid; else lo = mid + 1;
    }
    return (double)lo;
}

// dimension d of candidate g from component k: the label's value (after the
// exp of a log kind; Q: and the rounding to the grid of a quantized dimension,
// or the category of a categorical one)
template <bool Q, bool C = Q>
__device__ __forceinline__ double jdraw(const JP& p, const JDim& j, int d, int k, uint32_t k0, uint32_t k1,
                                        uint32_t g, uint32_t round) {
    if constexpr (C)
        if (j.upper > 0) return jdraw_cat(p, j, d, k, k0, k1, g, round);
    const DLabel L = jlabel(j);
    uint32_t wp, wu;
    draw_words(L, k0, k1, g, round, wp, wu);
    const JDraw r = p.draw[(size_t)k * p.D + d];
    DrawComp c;
    c.mu = r.mu;
    c.ssg = r.ssg;
    c.p0 = r.p0;
    c.q0 = r.q0;
    c.m = r.m;
    c.iw = 0x1.0p-32;
    c.tlo = 0;
    c.thi = 1ull << 32;
    const double y = icdf_draw(L, c, wp, wu);
    const double v = j.log ? lgmm_value(y) : y;
    if constexpr (Q)
        if (j.q > 0.0) return quantize(v, j.q);
    return v;
}

__global__ __launch_bounds__(kJBlock) void k_joint_draw(JP p, int64_t n, int64_t cand_offset, uint64_t seed,
                                                        uint32_t round, double* __restrict__ values,
                                                        int32_t* __restrict__ comp, int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * kJBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), g = (uint32_t)(cand_offset + i);
    const int k = jpick(p, k0, k1, g, round);
    comp[i] = k;
    bool bad = false;
    for (int d = 0; d < p.D; ++d) {
        const double x = jdraw<true>(p, p.dims[d], d, k, k0, k1, g, round);
        bad |= x != x;
        values[(size_t)i * p.D + d] = x;
    }
    if (bad) atomicOr(err, 1);
}

// ----------------------------------------------------------------- score ----
template <bool TABC>
__device__ __forceinline__ double jexp(double u, const double* __restrict__ tab) {
    // (beyond -8e6 the result is 0 either way; the clamp keeps rint(u) an int)
    return exp_scaled(fmax(u, -8.0e6), TABC ? kExp2Tab : tab);
}

// (max, sum) of exp(E_k - max) over components [k0, k1), online in groups of
// kJU; an empty or all -inf range gives (-inf, 0).  DR > 0: y' in yr (D <= DR),
// else in LDS at yl[d * kJLdsLanes].
template <int DR, bool TABC>
__device__ __forceinline__ void slice_ms(const double2* __restrict__ rec, const double* __restrict__ cst, int D,
                                         int k0, int k1, const double* yr, const double* yl,
                                         const double* __restrict__ tab, double& m, double& s) {
#pragma clang fp contract(off)
    m = -kInf;
    s = 0.0;
    for (int k = k0; k < k1; k += kJU) {
        const double2* r[kJU];
        double acc[kJU];
#pragma unroll
        for (int j = 0; j < kJU; ++j) {
            r[j] = rec + (size_t)min(k + j, k1 - 1) * D;
            acc[j] = 0.0;
        }
        if constexpr (DR > 0) {
#pragma unroll
            for (int d = 0; d < DR; ++d)
                if (d < D) {
                    const double y = yr[d];
#pragma unroll
                    for (int j = 0; j < kJU; ++j) {
                        const double2 q = r[j][d];
                        const double z = fma(y, q.y, -q.x);
                        acc[j] = fma(z, z, acc[j]);
                    }
                }
        } else {
            for (int d = 0; d < D; ++d) {
                const double y = yl[d * kJLdsLanes];
#pragma unroll
                for (int j = 0; j < kJU; ++j) {
                    const double2 q = r[j][d];
                    const double z = fma(y, q.y, -q.x);
                    acc[j] = fma(z, z, acc[j]);
                }
            }
        }
        double e[kJU], gm = -kInf;
#pragma unroll
        for (int j = 0; j < kJU; ++j) {
            e[j] = (k + j < k1) ? cst[min(k + j, k1 - 1)] - acc[j] : -kInf;
            gm = fmax(gm, e[j]);
        }
        const double M = fmax(m, gm);
        if (M > -kInf) {
            double t = (m > -kInf) ? s * jexp<TABC>(m - M, tab) : 0.0;
#pragma unroll
            for (int j = 0; j < kJU; ++j)
                if (e[j] > -kInf) t += jexp<TABC>(e[j] - M, tab);
            s = t;
            m = M;
        }
    }
}

// Phi(zu sqrt 2) - Phi(zl sqrt 2), the normal mass of a quantized value's
// interval, from the side it lies on: two upper (or, mirrored, lower) tails
// when both ends are on one side of the mean, two positive erf terms when it
// straddles the mean -- never a difference of values near 1/2 or 1.  An empty
// interval has mass 0 (a NaN end too: the candidate's ylog carries the NaN).
__device__ __forceinline__ double jmass(double zl, double zu) {
#pragma clang fp contract(off)
    if (!(zu > zl)) return 0.0;
    if (zl >= 0.0 || zu <= 0.0) {
        const double a = zl >= 0.0 ? zl : -zu, b = zl >= 0.0 ? zu : -zl;
        return 0.5 * (erfc(a) - erfc(b));
    }
    return 0.5 * (erf(zu) + erf(-zl));
}

// slice_ms of a group with quantized dimensions; the per-candidate values are
// in LDS at yl[slot * kJLdsLanes]: y' of a dense dimension in its slot, the
// interval ends (ub', lb') of a quantized one in its slot and the next.  The
// quantized factors of a component multiply into a mantissa in [1/2, 1) and an
// integer exponent (60 fine-grid factors are below 1e-320 together); one log
// per component folds them into E_k.  A zero factor: E_k = -inf.
// C: the group may hold categorical dimensions -- the candidate's category in
// the dimension's slot (-2: none), the record (o_kd, -K bonus): a hit adds the
// bonus to E_k.
template <bool TABC, bool C = false>
__device__ __forceinline__ void slice_ms_q(const JDim* __restrict__ dims, const double2* __restrict__ rec,
                                           const double* __restrict__ cst, int D, int k0, int k1, const double* yl,
                                           const double* __restrict__ tab, double& m, double& s) {
#pragma clang fp contract(off)
    m = -kInf;
    s = 0.0;
    for (int k = k0; k < k1; k += kJU) {
        const double2* r[kJU];
        double acc[kJU], mant[kJU];
        int ex[kJU];
#pragma unroll
        for (int j = 0; j < kJU; ++j) {
            r[j] = rec + (size_t)min(k + j, k1 - 1) * D;
            acc[j] = 0.0;
            mant[j] = 1.0;
            ex[j] = 0;
        }
        for (int d = 0; d < D; ++d) {
            const int sl = dims[d].slot;
            if constexpr (C)
                if (dims[d].upper > 0) {
                    const double y = yl[sl * kJLdsLanes];
#pragma unroll
                    for (int j = 0; j < kJU; ++j) {
                        const double2 q = r[j][d];
                        acc[j] += y == q.x ? q.y : 0.0;
                    }
                    continue;
                }
            if (dims[d].q > 0.0) {
                const double u = yl[sl * kJLdsLanes], l = yl[(sl + 1) * kJLdsLanes];
#pragma unroll
                for (int j = 0; j < kJU; ++j) {
                    const double2 q = r[j][d];
                    const double g = jmass(fma(l, q.y, -q.x), fma(u, q.y, -q.x));
                    int e;
                    mant[j] = frexp(mant[j] * g, &e);
                    ex[j] += e;
                }
            } else {
                const double y = yl[sl * kJLdsLanes];
#pragma unroll
                for (int j = 0; j < kJU; ++j) {
                    const double2 q = r[j][d];
                    const double z = fma(y, q.y, -q.x);
                    acc[j] = fma(z, z, acc[j]);
                }
            }
        }
        double e[kJU], gm = -kInf;
#pragma unroll
        for (int j = 0; j < kJU; ++j) {
            const double lq = (log(mant[j]) + (double)ex[j] * 0.69314718055994530942) * kExpScale;
            e[j] = (k + j < k1) ? (cst[min(k + j, k1 - 1)] - acc[j]) + lq : -kInf;
            gm = fmax(gm, e[j]);
        }
        const double M = fmax(m, gm);
        if (M > -kInf) {
            double t = (m > -kInf) ? s * jexp<TABC>(m - M, tab) : 0.0;
#pragma unroll
            for (int j = 0; j < kJU; ++j)
                if (e[j] > -kInf) t += jexp<TABC>(e[j] - M, tab);
            s = t;
            m = M;
        }
    }
}

template <bool TABC>
__device__ __forceinline__ void ms_merge(double& m, double& s, double m2, double s2,
                                         const double* __restrict__ tab) {
#pragma clang fp contract(off)
    if (!(m2 > -kInf)) return;
    if (!(m > -kInf)) {
        m = m2;
        s = s2;
        return;
    }
    const double M = fmax(m, m2);
    const double t1 = s * jexp<TABC>(m - M, tab), t2 = s2 * jexp<TABC>(m2 - M, tab);
    s = t1 + t2;
    m = M;
}

// lpdf of one side from its merged (max, sum); ylog = sum of the log kinds'
// y_d, NaN when a value is NaN
__device__ __forceinline__ double jfinish(double m, double s, double logA, double ylog) {
#pragma clang fp contract(off)
    const double lse = (m > -kInf) ? flog(s) + m * kExpScaleInv : -kInf;
    return (lse - logA) - ylog;
}

__device__ __forceinline__ int jslices(int K) { return (K + kJSlice - 1) / kJSlice; }

// the best (key, index) of a workgroup with its lpdfs -> *out (thread 0)
// (scratch: 32 bytes of LDS per thread, free for reuse)
__device__ __forceinline__ void jblock_best(uint64_t key, int64_t idx, double ll, double lg, Partial* out,
                                            double* scratch) {
    const int t = threadIdx.x, nt = blockDim.x;
    uint64_t* skey = reinterpret_cast<uint64_t*>(scratch);
    int64_t* sidx = reinterpret_cast<int64_t*>(scratch + nt);
    double *sll = scratch + 2 * nt, *slg = scratch + 3 * nt;
    skey[t] = key;
    sidx[t] = idx;
    sll[t] = ll;
    slg[t] = lg;
    __syncthreads();
    for (int w = nt >> 1; w > 0; w >>= 1) {
        if (t < w && better(skey[t + w], sidx[t + w], skey[t], sidx[t])) {
            skey[t] = skey[t + w];
            sidx[t] = sidx[t + w];
            sll[t] = sll[t + w];
            slg[t] = slg[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        Partial r;
        r.key = skey[0];
        r.idx = sidx[0];
        r.value = 0.0;
        r.lb = sll[0];
        r.la = slg[0];
        *out = r;
    }
}

// (rec and cst are the posterior's records again, as plain read-only kernel
// arguments: the compiler then reads them through the scalar unit)
// grid (tiles, 1): the whole round of a tile; grid (tiles, slices): one slice
// per workgroup, its (max, sum) to part[slice][i] and the candidate's ylog to
// aux[i] (k_joint_merge finishes).  SAMPLE: candidate i is drawn (index
// cand_offset + i), else read from vals[i][d].  Packed (rounds != nullptr): i
// is the flat index over rounds of ncell candidates each -- candidate
// cand_offset + i % ncell of round rounds[i / ncell]; every candidate's lpdfs are stored, and
// without `partials` no workgroup best is formed.
// Q: a group with quantized dimensions -- the LDS layout of slice_ms_q (DR = 0);
// C: that layout with categorical dimensions.
template <int DR, bool TABC, bool SAMPLE, bool Q = false, bool C = false>
__global__ __launch_bounds__(DR > 0 ? kJBlock : kJLdsLanes) void k_joint_round(
    JP p, const double2* __restrict__ rec, const double* __restrict__ cst, const double* __restrict__ vals, int64_t n, int64_t cand_offset, uint64_t seed, uint32_t round,
    const uint32_t* __restrict__ rounds, uint32_t ncell, int32_t split, double2* __restrict__ part, double* __restrict__ aux, double* __restrict__ out_ll,
    double* __restrict__ out_lg, Partial* __restrict__ partials, int32_t* __restrict__ err) {
    static_assert(!Q || DR == 0, "quantized groups keep their values in LDS");
    static_assert(!C || Q, "categorical dimensions run the quantized variant");
    extern __shared__ double jsm[];
    const double* tab = jsm;
    if constexpr (!TABC) load_exp_table(jsm);
    double* yl = jsm + (TABC ? 0 : kExpTabSize) + threadIdx.x;
    constexpr int NR = DR > 0 ? DR : 1;
    double yr[NR];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    const int D = p.D;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t g = (uint32_t)(cand_offset + i);
    if (rounds && valid) {   // (n < 2^31 in packed launches)
        const uint32_t r = (uint32_t)i / ncell;
        g = (uint32_t)cand_offset + ((uint32_t)i - r * ncell);
        round = rounds[r];
    }
    int kc = 0;
    if constexpr (SAMPLE)
        if (valid) kc = jpick(p, k0, k1, g, round);
    double ylog = 0.0;
    bool bad = false;
    auto load = [&](int d) -> double {
        const JDim j = p.dims[d];
        double y = j.centre;
        if (valid) {
            double x;
            if constexpr (SAMPLE) {
                x = jdraw<false>(p, j, d, kc, k0, k1, g, round);
                if (x != x) atomicOr(err, 1);
            } else {
                x = vals[(size_t)i * D + d];
            }
            y = j.log ? flog(x) : x;
            if (j.log) ylog += y;
            bad |= y != y;
        }
        return y - j.centre;
    };
    if constexpr (Q) {
        // a quantized dimension: the ends of the value's interval in the
        // working space (quant_bounds: the log of a log kind taken here, once
        // per candidate), recentred like y'; no Jacobian term
        bool inval = false;
        for (int d = 0; d < D; ++d) {
            const JDim j = p.dims[d];
            if constexpr (C)
                if (j.upper > 0) {
                    // the category itself; its log p_d[x] leaves through ylog
                    // (the same on both sides), no integer in [0, C_d): factor 0
                    double c = -2.0;
                    if (valid) {
                        double x;
                        if constexpr (SAMPLE) x = jdraw_cat(p, j, d, kc, k0, k1, g, round);
                        else x = vals[(size_t)i * D + d];
                        if (x != x) {
                            bad = true;
                        } else if (x >= 0.0 && x < (double)j.upper && x == floor(x)) {
                            c = x;
                            ylog -= p.catlp[j.cat_off + (int)x];
                        } else {
                            inval = true;
                        }
                    }
                    yl[j.slot * kJLdsLanes] = c;
                    continue;
                }
            if (!(j.q > 0.0)) {
                yl[j.slot * kJLdsLanes] = load(d);
                continue;
            }
            double ub = j.centre, lb = j.centre;
            if (valid) {
                double x;
                if constexpr (SAMPLE) {
                    x = jdraw<true, false>(p, j, d, kc, k0, k1, g, round);
                    if (x != x) atomicOr(err, 1);
                } else {
                    x = vals[(size_t)i * D + d];
                }
                DLabel L{};
                L.flags = j.flags;
                L.q = j.q;
                L.low = j.low;
                L.high = j.high;
                L.exp_low = j.elo;
                L.exp_high = j.ehi;
                bool neg;
                if (j.log) quant_bounds<QUANT_LGMM>(L, x, ub, lb, neg);
                else quant_bounds<QUANT_GMM>(L, x, ub, lb, neg);
                bad |= x != x;
            }
            yl[j.slot * kJLdsLanes] = ub - j.centre;
            yl[(j.slot + 1) * kJLdsLanes] = lb - j.centre;
        }
        if constexpr (C)
            if (inval) ylog = kInf;
        yr[0] = 0.0;
    } else if constexpr (DR > 0) {
        // (the draw stays a loop: placed by selects, one copy of its code)
#pragma unroll
        for (int e = 0; e < DR; ++e) yr[e] = 0.0;
        for (int d = 0; d < D; ++d) {
            const double y = load(d);
#pragma unroll
            for (int e = 0; e < DR; ++e) yr[e] = e == d ? y : yr[e];
        }
    } else {
        for (int d = 0; d < D; ++d) yl[d * kJLdsLanes] = load(d);
        yr[0] = 0.0;
    }
    if (bad) ylog = __builtin_nan("");
    const int nsb = jslices(p.Kb);
    if (split) {
        const int sl = blockIdx.y;
        const bool above = sl >= nsb;
        const int K = above ? p.Ka : p.Kb, base = above ? p.Kb : 0, q = above ? sl - nsb : sl;
        const int a0 = q * kJSlice, a1 = min(a0 + kJSlice, K);
        double m, s;
        if constexpr (Q) slice_ms_q<TABC, C>(p.dims, rec, cst, D, base + a0, base + a1, yl, tab, m, s);
        else slice_ms<DR, TABC>(rec, cst, D, base + a0, base + a1, yr, yl, tab, m, s);
        if (valid) {
            part[(size_t)sl * n + i] = make_double2(m, s);
            if (sl == 0) aux[i] = ylog;
        }
        return;
    }
    double lp[2];
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        const int K = side ? p.Ka : p.Kb, base = side ? p.Kb : 0;
        double m = -kInf, s = 0.0;
        for (int a0 = 0; a0 < K; a0 += kJSlice) {
            double m2, s2;
            if constexpr (Q)
                slice_ms_q<TABC, C>(p.dims, rec, cst, D, base + a0, base + min(a0 + kJSlice, K), yl, tab, m2, s2);
            else
                slice_ms<DR, TABC>(rec, cst, D, base + a0, base + min(a0 + kJSlice, K), yr, yl, tab, m2, s2);
            ms_merge<TABC>(m, s, m2, s2, tab);
        }
        lp[side] = jfinish(m, s, p.logA[side], ylog);
    }
    if (out_ll && valid) {
        out_ll[i] = lp[0];
        out_lg[i] = lp[1];
    }
    if (!partials) return;
    __syncthreads();   // (the table and y' are done with: their LDS is the reduction's)
    jblock_best(valid ? order_key(lp[0] - lp[1]) : 0ull, valid ? i : INT64_MAX, lp[0], lp[1],
                partials + blockIdx.x, jsm);
}

__global__ __launch_bounds__(kJBlock) void k_joint_merge(JP p, int64_t n, const double2* __restrict__ part,
                                                         const double* __restrict__ aux,
                                                         double* __restrict__ out_ll, double* __restrict__ out_lg,
                                                         Partial* __restrict__ partials) {
    const int64_t i = (int64_t)blockIdx.x * kJBlock + threadIdx.x;
    const bool valid = i < n;
    const int nsb = jslices(p.Kb), nsa = jslices(p.Ka);
    double lp[2] = {0.0, 0.0};
    if (valid) {
        const double ylog = aux[i];
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const int s0 = side ? nsb : 0, s1 = side ? nsb + nsa : nsb;
            double m = -kInf, s = 0.0;
            for (int sl = s0; sl < s1; ++sl) {
                const double2 q = part[(size_t)sl * n + i];
                ms_merge<true>(m, s, q.x, q.y, nullptr);
            }
            lp[side] = jfinish(m, s, p.logA[side], ylog);
        }
        if (out_ll) {
            out_ll[i] = lp[0];
            out_lg[i] = lp[1];
        }
    }
    if (!partials) return;
    __shared__ double scr[4 * kJBlock];
    jblock_best(valid ? order_key(lp[0] - lp[1]) : 0ull, valid ? i : INT64_MAX, lp[0], lp[1],
                partials + blockIdx.x, scr);
}

// res: lpdf_below, lpdf_above, global index (cand_offset + the winner's
// position in the launch), then (SAMPLE rounds) the winner's D values
__global__ __launch_bounds__(kJBlock) void k_joint_best(JP p, const Partial* __restrict__ partials, int32_t nparts,
                                                        int64_t cand_offset, uint64_t seed, uint32_t round,
                                                        int32_t sample, double* __restrict__ res) {
    uint64_t bk = 0;
    int64_t bi = INT64_MAX;
    double ll = 0.0, lg = 0.0;
    for (int j = threadIdx.x; j < nparts; j += kJBlock) {
        const Partial q = partials[j];
        if (better(q.key, q.idx, bk, bi)) {
            bk = q.key;
            bi = q.idx;
            ll = q.lb;
            lg = q.la;
        }
    }
    __shared__ Partial win;
    __shared__ double scr[4 * kJBlock];
    jblock_best(bk, bi, ll, lg, &win, scr);
    __syncthreads();
    const Partial w = win;
    if (threadIdx.x == 0) {
        res[0] = w.lb;
        res[1] = w.la;
        res[2] = w.idx == INT64_MAX ? (double)w.idx : (double)(cand_offset + w.idx);
    }
    if (!sample || w.idx == INT64_MAX) return;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), g = (uint32_t)(cand_offset + w.idx);
    const int kc = jpick(p, k0, k1, g, round);
    for (int d = threadIdx.x; d < p.D; d += kJBlock) res[3 + d] = jdraw<true>(p, p.dims[d], d, kc, k0, k1, g, round);
}

// packed rounds: workgroup b reduces the ncell (ll, lg) pairs of round slot b
// with k_joint_round's key and order, and writes the slot's row like
// k_joint_best: lpdf_below, lpdf_above, global index, the winner's D values
// (candidate j of a cell is cand_offset + j of its round)
__global__ __launch_bounds__(kJBlock) void k_joint_best_cells(JP p, const double* __restrict__ ll,
                                                              const double* __restrict__ lg,
                                                              const uint32_t* __restrict__ rounds, uint32_t ncell,
                                                              int64_t cand_offset, uint64_t seed,
                                                              double* __restrict__ res) {
    const size_t base = (size_t)blockIdx.x * ncell;
    uint64_t bk = 0;
    int64_t bi = INT64_MAX;
    double bl = 0.0, bg = 0.0;
    for (uint32_t j = threadIdx.x; j < ncell; j += kJBlock) {
        const double a = ll[base + j], b = lg[base + j];
        const uint64_t key = order_key(a - b);
        if (better(key, (int64_t)j, bk, bi)) {
            bk = key;
            bi = (int64_t)j;
            bl = a;
            bg = b;
        }
    }
    __shared__ Partial win;
    __shared__ double scr[4 * kJBlock];
    jblock_best(bk, bi, bl, bg, &win, scr);
    __syncthreads();
    const Partial w = win;
    double* row = res + (size_t)blockIdx.x * (3 + p.D);
    if (threadIdx.x == 0) {
        row[0] = w.lb;
        row[1] = w.la;
        row[2] = w.idx == INT64_MAX ? (double)w.idx : (double)(cand_offset + w.idx);
    }
    if (w.idx == INT64_MAX) return;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), g = (uint32_t)(cand_offset + w.idx),
                   round = rounds[blockIdx.x];
    const int kc = jpick(p, k0, k1, g, round);
    for (int d = threadIdx.x; d < p.D; d += kJBlock) row[3 + d] = jdraw<true>(p, p.dims[d], d, kc, k0, k1, g, round);
}

// ------------------------------------------------------------- condition ----
// tpe_joint_condition_group: a slot's mixtures given the values of some of its
// dimensions F.  Each side's conditional over the free dimensions R keeps its
// components' means and sigmas; the weights become
//   L_k = log W_k + sum_{d in F} log g_kd(x_d),   W'_k = max(exp(L_k - lse), 2^-1022),
// g_kd the factor the round scores for the dimension: phi(y_d; mu_kd, s_kd) of a
// dense one (the Jacobian of a log kind is the same for every k and cancels),
// the mass of the value's rounding interval (quant_bounds, jmass on the fold's
// record) of a quantized one, r_kd[x_d] of a categorical one.  The floor keeps
// log W'_k finite for the fold.  A_S and the thresholds are the fold's, over R.
struct JFix {
    double x;     // the value as documents carry it
    int32_t d;    // its dimension in the source slot
    int32_t pad;
};

// one thread per component, both sides: L[k]
__global__ __launch_bounds__(kJBlock) void k_joint_cond_logw(const JDim* __restrict__ dims, int32_t D, int32_t Kb,
                                                             int32_t Ka, const double* __restrict__ W,
                                                             const double* __restrict__ mu,
                                                             const double* __restrict__ sig,
                                                             const JFix* __restrict__ fix, int32_t nf, double pw,
                                                             const double* __restrict__ ctab, int32_t ncat,
                                                             double* __restrict__ L) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * kJBlock + threadIdx.x;
    if (k >= Kb + Ka) return;
    double l = log(W[k]);
    for (int f = 0; f < nf; ++f) {
        const JFix t = fix[f];
        const JDim j = dims[t.d];
        const size_t o = (size_t)k * D + t.d;
        const double x = t.x;
        if (j.upper > 0) {   // r_kd[x]: log p[x] + log(a / (1 + a)) + [x == o_kd] log1p(1 / (a p[o_kd]))
            if (!(x >= 0.0 && x < (double)j.upper && x == floor(x))) {
                l = -kInf;
                continue;
            }
            const double* __restrict__ p = ctab + j.cat_off;
            const double* __restrict__ lp = ctab + 2 * (size_t)ncat + j.cat_off;
            double lr = lp[(int)x];
            if (k != 0 && k != Kb) {
                const double a = (double)j.upper * pw / (double)(k < Kb ? Kb : Ka);
                const double c = mu[o];
                lr -= log1p(1.0 / a);
                if (x == c) lr += log1p(1.0 / (a * p[(int)c]));
            }
            l += lr;
            continue;
        }
        const double s = sig[o], m = mu[o];
        if (j.q > 0.0) {
            DLabel Lb{};
            Lb.flags = j.flags;
            Lb.q = j.q;
            Lb.low = j.low;
            Lb.high = j.high;
            Lb.exp_low = j.elo;
            Lb.exp_high = j.ehi;
            double ub, lb;
            bool neg;
            if (j.log) quant_bounds<QUANT_LGMM>(Lb, x, ub, lb, neg);
            else quant_bounds<QUANT_GMM>(Lb, x, ub, lb, neg);
            const double a = 0.70710678118654752440 / s, mr = (m - j.centre) * a;   // the fold's record
            l += log(jmass(fma(lb - j.centre, a, -mr), fma(ub - j.centre, a, -mr)));
        } else {
            const double y = j.log ? flog(x) : x;
            const double z = (y - m) / s;
            l += -0.5 * (z * z) - log(s * 2.50662827463100050242);
        }
    }
    L[k] = l == l ? l : -kInf;   // (a value outside a log kind's support: no component reaches it)
}

// block b: side b's lse = L_max + log(sum_k exp(L_k - L_max)) over one fixed
// tree (strided partials in component order, then halving), and W'_k; a side
// whose every L_k is -inf stores 1 to refused[b] and writes no weight
__global__ __launch_bounds__(kJBlock) void k_joint_cond_weights(const double* __restrict__ L, int32_t Kb, int32_t Ka,
                                                                double* __restrict__ Wout,
                                                                int32_t* __restrict__ refused) {
#pragma clang fp contract(off)
    const int side = blockIdx.x, K = side ? Ka : Kb, t = threadIdx.x;
    const double* Ls = L + (side ? Kb : 0);
    double* Ws = Wout + (side ? Kb : 0);
    __shared__ double sh[kJBlock];
    double a = -kInf;
    for (int k = t; k < K; k += kJBlock) a = fmax(a, Ls[k]);
    sh[t] = a;
    __syncthreads();
    for (int w = kJBlock / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] = fmax(sh[t], sh[t + w]);
        __syncthreads();
    }
    const double M = sh[0];
    __syncthreads();
    if (!(M > -kInf && M < kInf)) {
        if (t == 0) refused[side] = 1;
        return;
    }
    a = 0.0;
    for (int k = t; k < K; k += kJBlock) a += exp(Ls[k] - M);
    sh[t] = a;
    __syncthreads();
    for (int w = kJBlock / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    const double lse = M + log(sh[0]);
    for (int k = t; k < K; k += kJBlock) Ws[k] = fmax(exp(Ls[k] - lse), 0x1.0p-1022);
}

// the free columns of mu and sigma, [K][D] -> [K][Dr], bit for bit
__global__ __launch_bounds__(kJBlock) void k_joint_cond_cols(const double* __restrict__ mu,
                                                             const double* __restrict__ sig, int32_t D, int32_t Dr,
                                                             int64_t K, const int32_t* __restrict__ free_d,
                                                             double* __restrict__ mu_out,
                                                             double* __restrict__ sig_out) {
    const int64_t e = (int64_t)blockIdx.x * kJBlock + threadIdx.x;
    if (e >= K * Dr) return;
    const int64_t k = e / Dr;
    const size_t o = (size_t)k * D + free_d[e - k * Dr];
    mu_out[e] = mu[o];
    sig_out[e] = sig[o];
}

// ------------------------------------------------------------- host side ----
template <typename T>
using DevBuf = tpe_rt::DevBuf<T>;

struct JointState {   // one slot's folded posterior
    int32_t D = 0, Kb = 0, Ka = 0;
    int32_t S = 0;        // per-candidate values: D + the number of quantized dimensions
    bool quant = false;   // a quantized dimension: the Q instantiations of k_joint_round
    bool cat = false;     // a categorical dimension: the Q, C instantiations
    int32_t ncat = 0;     // entries of each categorical table
    uint32_t stream = TPE_JOINT_STREAM;
    bool ready = false, zero = false;
    // the layout as the host laid it out and the prior weight of its fold: what
    // tpe_joint_condition_group lays the free dimensions out from
    std::vector<JDim> hd;
    std::vector<double> hctab;
    double pw = 0.0;
    DevBuf<JDim> dims;
    DevBuf<double> W, mu, sig, cst, P, logA;
    DevBuf<double> ctab;   // categorical tables: p, its running sums, log p (ncat each)
    DevBuf<double2> rec;
    DevBuf<JDraw> draw;
    DevBuf<uint64_t> thr;
    JP jp() const {
        JP p;
        p.dims = dims.p;
        p.rec = rec.p;
        p.cst = cst.p;
        p.logA = logA.p;
        p.thr = thr.p;
        p.draw = draw.p;
        p.catP = cat ? ctab.p + ncat : nullptr;
        p.catlp = cat ? ctab.p + 2 * (size_t)ncat : nullptr;
        p.D = D;
        p.Kb = Kb;
        p.Ka = Ka;
        p.stream = stream;
        return p;
    }
};

struct JGDim {   // one dimension of one group of a device build (k_joint_gather)
    double *W, *mu, *sig;   // its destination: column d of D (the slot's arrays, or a column buffer's: 0 of 1)
    double fb, fa;          // TPE_JOINT_BW_SCOTT: the bandwidth factor of the group's below / above side
    int32_t label, group, d, D, Kb, Ka;
    int32_t upper;          // > 0: categorical
    int32_t flags;          // 1: the build holds this label's above order; 2: this dimension supplies W
};

struct JointGroups {   // a context's slots and the scratch they share (one stream: one user at a time)
    std::unique_ptr<JointState> slot[kJMaxGroups];
    DevBuf<double> vals, ll, lg, aux, res, bres;
    DevBuf<double2> part;
    DevBuf<int32_t> err, comp, berr;
    DevBuf<JGDim> gtask;                  // a device build: its gather's tasks
    DevBuf<tpe_rt::JointWTask> wtask;     // under TPE_JOINT_BW_SCOTT: its weight columns
    DevBuf<double> bleaf;                 //   and their sums' scratch
    DevBuf<double> bcols;   // the build under label shards: the call's columns
    DevBuf<JFix> cfix;                    // tpe_joint_condition_group: the fixed dimensions,
    DevBuf<int32_t> cfree, cerr;          //   the free ones, a side's refusal,
    DevBuf<double> cL, cW, cmu, csig;     //   L_k, W'_k and the free columns
    DevBuf<Partial> partials;
    DevBuf<uint32_t> rounds;
    std::vector<double> hres;
};

JointGroups* jgroups(tpe_ctx* ctx, bool make) {
    if (!ctx->joint && make) ctx->joint = std::shared_ptr<void>(new JointGroups(), [](void* q) {
        delete static_cast<JointGroups*>(q);
    });
    return static_cast<JointGroups*>(ctx->joint.get());
}

constexpr size_t kJPartBytes = (size_t)64 << 20;   // the split map's (max, sum) pairs at most
constexpr int64_t kJSplitTiles = 512;              // tiles from which one workgroup runs a tile's whole round
// flat candidates (rounds x candidates) of one packed launch at most: 16 B of
// lpdfs each, 16 MiB, beside at most kJPartBytes of the split map
constexpr int64_t kJFlatCap = (int64_t)1 << 20;

// the round of n candidates (drawn, or G->vals): lpdfs to G->ll / G->lg when
// `lpdfs`, per-workgroup bests to G->partials, *nparts of them.  Packed
// (rounds: device pointer to the round numbers, ncell candidates each, n =
// their flat count): every candidate's lpdfs, no bests
int launch_round(tpe_ctx* ctx, JointGroups* G, JointState* J, bool sample, int64_t n, int64_t cand_offset,
                 uint64_t seed, uint32_t round, bool lpdfs, int32_t* nparts, int32_t* err,
                 const uint32_t* rounds = nullptr, uint32_t ncell = 0, const double* vals_dev = nullptr) {
    const int D = J->D;
    const double* vals_in = vals_dev ? vals_dev : G->vals.p;   // supplied candidates: the caller's device array
    const bool qv = J->quant || J->cat;   // the quantized variant
    const int S = qv ? J->S : D;   // values a lane keeps in LDS (dr == 0)
    const int dr = qv ? 0 : (D <= kJRegSmall ? kJRegSmall : (D <= kJReg ? kJReg : 0));
    // (a quantized group reads the exp table from memory whatever its size: one
    // exp per component against two erfc-class evaluations per quantized
    // dimension, and a table per one-wave workgroup would leave the CU two waves)
    const bool tabc = dr == 0 && (qv || S > kJLdsTabD);
    const int threads = dr ? kJBlock : kJLdsLanes;
    const int64_t tiles = (n + threads - 1) / threads;
    const int64_t nsl = (J->Kb + kJSlice - 1) / kJSlice + (J->Ka + kJSlice - 1) / kJSlice;
    const bool split = tiles < kJSplitTiles && nsl > 2 && (size_t)nsl * n * sizeof(double2) <= kJPartBytes &&
                       nsl <= 65535;
    size_t lds = (tabc ? 0 : kExpTabSize * sizeof(double)) + (dr ? 0 : (size_t)S * kJLdsLanes * sizeof(double));
    if (qv) lds = std::max(lds, 4 * kJLdsLanes * sizeof(double));   // (jblock_best's scratch)
    const int64_t mtiles = (n + kJBlock - 1) / kJBlock;
    *nparts = (int32_t)(split ? mtiles : tiles);
    if (!rounds) HIPCHK(ctx, G->partials.reserve(*nparts));
    if (split) {
        HIPCHK(ctx, G->part.reserve((size_t)nsl * n));
        HIPCHK(ctx, G->aux.reserve(n));
    }
    if (lpdfs) {
        HIPCHK(ctx, G->ll.reserve(n));
        HIPCHK(ctx, G->lg.reserve(n));
    }
    const dim3 grid((unsigned)tiles, split ? (unsigned)nsl : 1u);
    double* oll = lpdfs ? G->ll.p : nullptr;
    double* olg = lpdfs ? G->lg.p : nullptr;
    Partial* parts = rounds ? nullptr : G->partials.p;
    const JP p = J->jp();
#define JLAUNCH(DR, TABC, ...)                                                                                  \
    do {                                                                                                        \
        if (sample)                                                                                             \
            hipLaunchKernelGGL((k_joint_round<DR, TABC, true __VA_ARGS__>), grid, dim3(threads), lds, ctx->stream, p, \
                               J->rec.p, J->cst.p, nullptr, n, cand_offset, seed, round, rounds, ncell,         \
                               (int32_t)split, G->part.p, G->aux.p, split ? nullptr : oll,                      \
                               split ? nullptr : olg, parts, err);                                              \
        else                                                                                                    \
            hipLaunchKernelGGL((k_joint_round<DR, TABC, false __VA_ARGS__>), grid, dim3(threads), lds, ctx->stream, p, \
                               J->rec.p, J->cst.p, vals_in, n, cand_offset, seed, round, rounds, ncell,         \
                               (int32_t)split, G->part.p, G->aux.p, split ? nullptr : oll,                      \
                               split ? nullptr : olg, parts, err);                                              \
    } while (0)
    if (J->cat) JLAUNCH(0, true, , true, true);
    else if (J->quant) JLAUNCH(0, true, , true);
    else if (dr == kJRegSmall) JLAUNCH(kJRegSmall, false);
    else if (dr == kJReg) JLAUNCH(kJReg, false);
    else if (!tabc) JLAUNCH(0, false);
    else JLAUNCH(0, true);
#undef JLAUNCH
    HIPCHK(ctx, hipGetLastError());
    if (split) {
        hipLaunchKernelGGL(k_joint_merge, dim3((unsigned)mtiles), dim3(kJBlock), 0, ctx->stream, p, n, G->part.p,
                           G->aux.p, oll, olg, parts);
        HIPCHK(ctx, hipGetLastError());
    }
    return TPE_OK;
}

int zero_mass(tpe_ctx* ctx) {
    return ctx->fail(TPE_ERR_SAMPLE, "truncated sampler: the box holds none of the below mixture's mass");
}

int joint_ready(tpe_ctx* ctx, int32_t slot, JointGroups** Gout, JointState** out, const char* who) {
    if (slot < 0 || slot >= kJMaxGroups)
        return ctx->fail(TPE_ERR_ARG, std::string(who) + ": slot must be in [0, " + std::to_string(kJMaxGroups) + ")");
    JointGroups* G = jgroups(ctx, false);
    JointState* J = G ? G->slot[slot].get() : nullptr;
    if (!J || !J->ready) return ctx->fail(TPE_ERR_ARG, std::string(who) + ": no joint posterior set");
    if (J->zero) return zero_mass(ctx);
    *Gout = G;
    *out = J;
    return TPE_OK;
}

int check_range(tpe_ctx* ctx, int64_t n, int64_t cand_offset) {
    if (n <= 0) return ctx->fail(TPE_ERR_ARG, "the number of candidates must be positive");
    if (cand_offset < 0 || cand_offset + n > (int64_t)UINT32_MAX)
        return ctx->fail(TPE_ERR_ARG, "candidate indices must stay below 2^32");
    return TPE_OK;
}

int not_reached(tpe_ctx* ctx) {
    return ctx->fail(TPE_ERR_SAMPLE, "truncated sampler: interval [low, high) not reached");
}

int read_err(tpe_ctx* ctx, JointGroups* G) {
    int32_t e = 0;
    HIPCHK(ctx, hipMemcpyAsync(&e, G->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (e & 1) return not_reached(ctx);
    return TPE_OK;
}

// ------------------------------------------------------ one group's slot ----
// Every path that puts a posterior into a slot -- the upload and the device
// builds -- lays the group out (joint_layout), reserves the slot's buffers
// (joint_reserve_slot), fills W / mu / sig, folds (joint_fold_group) and, after
// its synchronisation, records the slot (joint_commit).
struct JDimSpec {   // one dimension of a group as its caller describes it
    double low, high;   // bounds and their flags as the dimension's JDim holds them
    double prior_mu;    // the prior's mu: the dimension's centre
    double q;           // step of a quantized dimension, 0: dense
    int32_t flags;      // TPE_HAS_LOW | TPE_HAS_HIGH
    int32_t log;        // 1: a log kind
    int32_t C;          // categories, 0: not categorical (a categorical dimension's fields above are not read)
    int32_t stream;     // the label's Philox stream
};

struct GInfo {   // one validated group: its layout, and its side counts from the caller
    int32_t D, S, Kb, Ka, ncat;
    bool quant, cat;
    std::vector<JDim> hd;
    std::vector<double> ctab;   // categorical tables: p, its running sums in category order, log p (ncat each)
};

// the layout of the group of dimensions ds into I (all but Kb, Ka); cat_p: the
// group's categorical priors, one after the other
int joint_layout(tpe_ctx* ctx, const std::vector<JDimSpec>& ds, const double* cat_p, double prior_weight,
                 GInfo& I) {
    const int D = I.D = (int32_t)ds.size();
    int S = 0;
    size_t ncat = 0;   // categories of all categorical dimensions
    for (const JDimSpec& s : ds) {
        if (!(s.q >= 0.0 && s.q < __builtin_inf()))
            return ctx->fail(TPE_ERR_ARG, "a quantization step is finite and not negative (0: dense)");
        S += s.q > 0.0 ? 2 : 1;
        if (s.C < 0) return ctx->fail(TPE_ERR_ARG, "upper is the number of categories, 0: not categorical");
        if (s.C > 0 && s.q > 0.0)
            return ctx->fail(TPE_ERR_ARG, "a joint dimension is quantized or categorical, not both");
        ncat += (size_t)s.C;
    }
    if (S > kJMaxD)
        return ctx->fail(TPE_ERR_ARG, "a joint group holds at most " + std::to_string(kJMaxD) +
                                          " per-candidate values: dimensions plus quantized dimensions");
    if (ncat > (size_t)INT32_MAX / 4) return ctx->fail(TPE_ERR_ARG, "too many categories");
    I.S = S;
    I.quant = S > D;
    I.cat = ncat > 0;
    I.ncat = (int32_t)ncat;
    I.ctab.assign(3 * ncat, 0.0);
    if (I.cat) {
        if (!cat_p) return ctx->fail(TPE_ERR_ARG, "null pointer");
        if (!(prior_weight > 0.0 && prior_weight < __builtin_inf()))
            return ctx->fail(TPE_ERR_ARG, "a categorical dimension needs a positive finite prior weight");
    }
    size_t at = 0;
    for (const JDimSpec& s : ds) {
        double run = 0.0;
        for (int32_t c = 0; c < s.C; ++c, ++at) {
            const double pc = cat_p[at];
            if (!(pc > 0.0 && pc < __builtin_inf()))
                return ctx->fail(TPE_ERR_ARG, "a categorical prior's entries are positive and finite");
            run += pc;
            I.ctab[at] = pc;
            I.ctab[ncat + at] = run;
            I.ctab[2 * ncat + at] = std::log(pc);
        }
        if (s.C > 0 && !(std::fabs(run - 1.0) <= 1e-9)) return ctx->fail(TPE_ERR_ARG, "a categorical prior sums to 1");
    }
    I.hd.resize(D);
    for (int d = 0, vs = 0, coff = 0; d < D; ++d) {   // vs: the dimension's first per-candidate value
        const JDimSpec& s = ds[d];
        if (s.C > 0) {
            I.hd[d] = JDim{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, s.stream, 0, vs, s.C, coff};
            vs += 1;
            coff += s.C;
            continue;
        }
        if ((s.flags & 3) == 3 && !(s.low < s.high)) return ctx->fail(TPE_ERR_VALUE, "low >= high");
        I.hd[d] = JDim{s.low, s.high, s.prior_mu, s.q, s.log ? std::exp(s.low) : 0.0, s.log ? std::exp(s.high) : 0.0,
                       s.flags, s.stream, s.log, (I.quant || I.cat) ? vs : d, 0, 0};
        vs += s.q > 0.0 ? 2 : 1;
    }
    return TPE_OK;
}

// the slot of a group about to be filled: unset, its buffers at the group's size
int joint_reserve_slot(tpe_ctx* ctx, JointGroups* G, int32_t slot, const GInfo& I, JointState** out) {
    if (!G->slot[slot]) G->slot[slot].reset(new JointState());
    JointState* J = G->slot[slot].get();
    J->ready = false;
    const int D = I.D, Kb = I.Kb, K = I.Kb + I.Ka;
    HIPCHK(ctx, J->dims.reserve(D));
    HIPCHK(ctx, J->W.reserve(K));
    HIPCHK(ctx, J->mu.reserve((size_t)K * D));
    HIPCHK(ctx, J->sig.reserve((size_t)K * D));
    HIPCHK(ctx, J->rec.reserve((size_t)K * D));
    HIPCHK(ctx, J->cst.reserve(K));
    HIPCHK(ctx, J->P.reserve(K));
    HIPCHK(ctx, J->logA.reserve(2));
    HIPCHK(ctx, J->draw.reserve((size_t)Kb * D));
    HIPCHK(ctx, J->thr.reserve(Kb));
    if (I.cat) HIPCHK(ctx, J->ctab.reserve(I.ctab.size()));
    *out = J;
    return TPE_OK;
}

// queue the upload of the group's tables and records (the setter's go ahead of
// its large copies: a small copy behind them waits for them)
int joint_upload_layout(tpe_ctx* ctx, JointState* J, const GInfo& I) {
    hipStream_t st = ctx->stream;
    if (I.cat)
        HIPCHK(ctx, hipMemcpyAsync(J->ctab.p, I.ctab.data(), I.ctab.size() * sizeof(double), hipMemcpyHostToDevice,
                                   st));
    HIPCHK(ctx, hipMemcpyAsync(J->dims.p, I.hd.data(), I.D * sizeof(JDim), hipMemcpyHostToDevice, st));
    return TPE_OK;
}

// queue the fold of the slot's W / mu / sig under its uploaded layout; its error word: *err
int joint_fold_group(tpe_ctx* ctx, JointState* J, const GInfo& I, double prior_weight, int32_t* err) {
    hipStream_t st = ctx->stream;
    const int K = I.Kb + I.Ka;
    hipLaunchKernelGGL(k_joint_fold, dim3((K + kJBlock - 1) / kJBlock), dim3(kJBlock), 0, st, J->dims.p, I.D, I.Kb,
                       I.Ka, J->W.p, J->mu.p, J->sig.p, J->rec.p, J->cst.p, J->P.p, J->draw.p, prior_weight,
                       I.cat ? J->ctab.p : nullptr);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_joint_fold_sum, dim3(2), dim3(kJBlock), 0, st, J->P.p, I.Kb, I.Ka, J->logA.p, J->thr.p, err);
    HIPCHK(ctx, hipGetLastError());
    return TPE_OK;
}

// the slot's record after the caller's synchronisation (a group the device
// build flagged stays unset: it is the host build's)
void joint_commit(JointState* J, const GInfo& I, double prior_weight, uint32_t pick_stream, int32_t flag,
                  int32_t fold_err) {
    J->hd = I.hd;
    J->hctab = I.ctab;
    J->pw = prior_weight;
    J->D = I.D;
    J->S = I.S;
    J->quant = I.quant;
    J->cat = I.cat;
    J->ncat = I.ncat;
    J->Kb = I.Kb;
    J->Ka = I.Ka;
    J->stream = pick_stream;
    J->zero = (fold_err & 1) != 0;
    J->ready = flag == 0;
}

// upload and fold one slot's posterior (tpe_joint_set_group)
int joint_set(tpe_ctx* ctx, int32_t slot, uint32_t pick_stream, const tpe_joint_dim* dims, const double* q,
              const int32_t* upper, const double* cat_p, double prior_weight, int32_t n_dims, int32_t n_below,
              const double* wb, const double* mub, const double* sigb, int32_t n_above, const double* wa,
              const double* mua, const double* siga) {
    if (!ctx) return TPE_ERR_ARG;
    if (slot < 0 || slot >= kJMaxGroups)
        return ctx->fail(TPE_ERR_ARG, "a joint slot is in [0, " + std::to_string(kJMaxGroups) + ")");
    if (!dims || !wb || !mub || !sigb || !wa || !mua || !siga) return ctx->fail(TPE_ERR_ARG, "null pointer");
    if (n_dims < 1 || n_dims > kJMaxD)
        return ctx->fail(TPE_ERR_ARG, "a joint group holds 1 to " + std::to_string(kJMaxD) + " dimensions");
    if (n_below < 1 || n_below > kJMaxBelow || n_above < 1)
        return ctx->fail(TPE_ERR_ARG, "each side needs its prior component (below: at most " +
                                          std::to_string(kJMaxBelow) + ")");
    const int D = n_dims, Kb = n_below, Ka = n_above;
    GInfo I{};
    I.Kb = Kb;
    I.Ka = Ka;
    std::vector<JDimSpec> ds(D);
    for (int d = 0; d < D; ++d) {
        const tpe_joint_dim& s = dims[d];
        const int32_t C = upper ? upper[d] : 0;
        ds[d] = JDimSpec{s.low, s.high, mub[d], q ? q[d] : 0.0, s.flags, s.kind == TPE_LGMM1 ? 1 : 0, C, s.stream};
        if (C > 0) {   // (kind, flags and bounds of a categorical dimension are not read)
            for (int side = 0; side < 2; ++side) {   // the observed categories (row 0, the prior's, is ignored)
                const double* m = side ? mua : mub;
                for (int k = 1; k < (side ? Ka : Kb); ++k) {
                    const double o = m[(size_t)k * D + d];
                    if (!(o >= 0.0 && o < (double)C && o == std::floor(o)))
                        return ctx->fail(TPE_ERR_ARG, "an observed category is an integer in [0, upper)");
                }
            }
            continue;
        }
        if (s.kind != TPE_GMM1 && s.kind != TPE_LGMM1)
            return ctx->fail(TPE_ERR_ARG, "a joint dimension is TPE_GMM1 or TPE_LGMM1");
        if (s.flags & ~(TPE_HAS_LOW | TPE_HAS_HIGH)) return ctx->fail(TPE_ERR_ARG, "joint dimensions are not quantized");
    }
    int rc = joint_layout(ctx, ds, cat_p, prior_weight, I);
    if (rc) return rc;
    for (int side = 0; side < 2; ++side) {
        const double *w = side ? wa : wb, *sg = side ? siga : sigb;
        const int Ks = side ? Ka : Kb;
        for (int k = 0; k < Ks; ++k)
            if (!(w[k] >= 0.0)) return ctx->fail(TPE_ERR_VALUE, "negative or NaN weight");
        for (size_t o = 0; o < (size_t)Ks * D; ++o)
            if (!(I.cat && ds[o % D].C > 0) && !(sg[o] > 0.0 && sg[o] < __builtin_inf()))
                return ctx->fail(TPE_ERR_VALUE, "sigma must be positive");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    JointGroups* G = jgroups(ctx, true);
    JointState* J = nullptr;
    if ((rc = joint_reserve_slot(ctx, G, slot, I, &J))) return rc;
    HIPCHK(ctx, G->err.reserve(1));
    hipStream_t st = ctx->stream;
    if ((rc = joint_upload_layout(ctx, J, I))) return rc;
    const size_t nb = (size_t)Kb * D, na = (size_t)Ka * D;
    HIPCHK(ctx, hipMemcpyAsync(J->W.p, wb, Kb * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(J->W.p + Kb, wa, Ka * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(J->mu.p, mub, nb * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(J->mu.p + nb, mua, na * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(J->sig.p, sigb, nb * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(J->sig.p + nb, siga, na * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(G->err.p, 0, sizeof(int32_t), st));
    if ((rc = joint_fold_group(ctx, J, I, prior_weight, G->err.p))) return rc;
    int32_t e = 0;
    HIPCHK(ctx, hipMemcpyAsync(&e, G->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    joint_commit(J, I, prior_weight, pick_stream, 0, e);   // (set also when the box holds no below mass: the rounds refuse it)
    if (J->zero) return zero_mass(ctx);
    return TPE_OK;
}

// condition one slot on the values of some of its dimensions
// (tpe_joint_condition_group).  Two phases: W' and the free columns into the
// shared scratch, with the sides' refusals read back -- nothing of a slot is
// touched before they are known -- then the destination is laid out, filled
// from the scratch device to device and folded like any other slot.
int joint_condition(tpe_ctx* ctx, int32_t src_slot, int32_t dst_slot, int32_t n_fixed, const int32_t* fdims,
                    const double* values) {
    if (!ctx) return TPE_ERR_ARG;
    if (src_slot < 0 || src_slot >= kJMaxGroups || dst_slot < 0 || dst_slot >= kJMaxGroups)
        return ctx->fail(TPE_ERR_ARG, "a joint slot is in [0, " + std::to_string(kJMaxGroups) + ")");
    JointGroups* G = jgroups(ctx, false);
    JointState* S = G ? G->slot[src_slot].get() : nullptr;
    if (!S || !S->ready) return ctx->fail(TPE_ERR_ARG, "tpe_joint_condition_group: no joint posterior set");
    if (!fdims || !values) return ctx->fail(TPE_ERR_ARG, "null pointer");
    const int D = S->D, Kb = S->Kb, Ka = S->Ka, K = Kb + Ka;
    if (n_fixed < 1 || n_fixed > D - 1)
        return ctx->fail(TPE_ERR_ARG, "tpe_joint_condition_group: 1 to n_dims - 1 dimensions are fixed");
    std::vector<uint8_t> fixed(D, 0);
    std::vector<JFix> fix(n_fixed);
    for (int f = 0; f < n_fixed; ++f) {
        const int32_t d = fdims[f];
        if (d < 0 || d >= D || fixed[d])
            return ctx->fail(TPE_ERR_ARG, "tpe_joint_condition_group: fixed dimensions are distinct and in [0, n_dims)");
        fixed[d] = 1;
        fix[f] = JFix{values[f], d, 0};
    }
    for (int f = 0; f < n_fixed; ++f)
        if (values[f] != values[f]) return ctx->fail(TPE_ERR_VALUE, "tpe_joint_condition_group: a fixed value is NaN");
    // the free dimensions in their source order, laid out as a group of their own
    const double pw = S->pw;
    const uint32_t pick = S->stream;
    std::vector<int32_t> free_d;
    std::vector<JDimSpec> ds;
    std::vector<double> cat_p;
    for (int d = 0; d < D; ++d) {
        if (fixed[d]) continue;
        const JDim& j = S->hd[d];
        free_d.push_back(d);
        ds.push_back(JDimSpec{j.low, j.high, j.centre, j.q, j.flags, j.log, j.upper, j.stream});
        for (int32_t c = 0; c < j.upper; ++c) cat_p.push_back(S->hctab[j.cat_off + c]);
    }
    const int Dr = D - n_fixed;
    GInfo I{};
    I.Kb = Kb;
    I.Ka = Ka;
    int rc = joint_layout(ctx, ds, cat_p.empty() ? nullptr : cat_p.data(), pw, I);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, G->err.reserve(1));
    HIPCHK(ctx, G->cfix.reserve(n_fixed));
    HIPCHK(ctx, G->cfree.reserve(Dr));
    HIPCHK(ctx, G->cerr.reserve(2));
    HIPCHK(ctx, G->cL.reserve(K));
    HIPCHK(ctx, G->cW.reserve(K));
    HIPCHK(ctx, G->cmu.reserve((size_t)K * Dr));
    HIPCHK(ctx, G->csig.reserve((size_t)K * Dr));
    HIPCHK(ctx, hipMemcpyAsync(G->cfix.p, fix.data(), n_fixed * sizeof(JFix), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(G->cfree.p, free_d.data(), Dr * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(G->cerr.p, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_joint_cond_logw, dim3((K + kJBlock - 1) / kJBlock), dim3(kJBlock), 0, st, S->dims.p, D, Kb, Ka,
                       S->W.p, S->mu.p, S->sig.p, G->cfix.p, n_fixed, pw, S->cat ? S->ctab.p : nullptr, S->ncat,
                       G->cL.p);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_joint_cond_weights, dim3(2), dim3(kJBlock), 0, st, G->cL.p, Kb, Ka, G->cW.p, G->cerr.p);
    HIPCHK(ctx, hipGetLastError());
    const int64_t cells = (int64_t)K * Dr;
    hipLaunchKernelGGL(k_joint_cond_cols, dim3((unsigned)((cells + kJBlock - 1) / kJBlock)), dim3(kJBlock), 0, st,
                       S->mu.p, S->sig.p, D, Dr, (int64_t)K, G->cfree.p, G->cmu.p, G->csig.p);
    HIPCHK(ctx, hipGetLastError());
    int32_t refused[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(refused, G->cerr.p, sizeof(refused), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (refused[0] || refused[1])
        return ctx->fail(TPE_ERR_VALUE, std::string("tpe_joint_condition_group: no component of the ") +
                                            (refused[0] ? "below" : "above") + " mixture reaches the fixed values");
    JointState* J = nullptr;   // (dst == src: the slot's own buffers, large enough as they are)
    if ((rc = joint_reserve_slot(ctx, G, dst_slot, I, &J))) return rc;
    if ((rc = joint_upload_layout(ctx, J, I))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(J->W.p, G->cW.p, K * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(J->mu.p, G->cmu.p, cells * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(J->sig.p, G->csig.p, cells * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(G->err.p, 0, sizeof(int32_t), st));
    if ((rc = joint_fold_group(ctx, J, I, pw, G->err.p))) return rc;
    int32_t e = 0;
    HIPCHK(ctx, hipMemcpyAsync(&e, G->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    joint_commit(J, I, pw, pick, 0, e);
    if (J->zero) return zero_mass(ctx);
    return TPE_OK;
}

// ------------------------------------------------- device-resident build ----
// tpe_joint_build_groups: the unfolded arrays W [K], mu and sig [K][D] of every
// group, gathered from the resident univariate build (tpe_build.hip) instead
// of uploaded.  posterior.joint_mixture is that build's per-label mixtures
// read back in trial order -- row 0 the prior, row t + 1 the side's t-th
// observation -- so one launch un-permutes them: a thread per (dimension,
// side, sorted slot) reads the slot's trial from the build's own map (the
// above list's rank beside the sorted keys, or the supplied np.argsort order;
// the <= kBuildMaxLF below values are ranked in place, as k_parzen ranks them)
// and stores the slot's (w, mu, sigma) in the trial's row.
//
// SCOTT (tpe_joint_build_groups_bw, TPE_JOINT_BW_SCOTT): every trial row of
// dimension d has the sigma clip(f psig_d, psig_d / min(100, 1 + K), psig_d),
// f = 0.2 n^(-1/(D+4)) of the side's n = K - 1 trials (computed on the host:
// tpe_joint_bandwidth_factor; the product and the quotient are single IEEE
// operations here), row 0 the prior's psig_d.  No sorted position enters: a
// thread stores the below value of its trial or the sorted key of its slot,
// the latter in the row of the build's rank map -- tied observations get equal
// rows whichever way the map orders them, so no tie flag.  The univariate
// w / sigma are not read (their pointers are null); W is k_joint_weights'
// (tpe_build.hip), launched beside this kernel.
//
// (fp contract(off) covers both instantiations: the neighbour rule's only
// floating-point operation is the 1.0 / Ks of a flagged row)
constexpr int32_t kJFlagTie = TPE_JOINT_FLAG_TIE, kJFlagCat = TPE_JOINT_FLAG_CATEGORY,
                  kJFlagCount = TPE_JOINT_FLAG_COUNT;
constexpr int32_t kJointLF = 25;   // linear_forgetting_weights(n, 25): posterior.DEFAULT_LF

template <bool SCOTT>
__global__ __launch_bounds__(kJBlock) void k_joint_gather(
    const JGDim* __restrict__ tasks, const tpe_label_spec* __restrict__ specs, const int64_t* __restrict__ p_off,
    const int32_t* __restrict__ counts, const double* __restrict__ below_val, const double* __restrict__ keys,
    const int32_t* __restrict__ idx, const int64_t* __restrict__ order_off, const int32_t* __restrict__ order,
    const int64_t* __restrict__ mix_off, const double* __restrict__ w, const double* __restrict__ sigma,
    int32_t* __restrict__ flags) {
#pragma clang fp contract(off)
    const JGDim t = tasks[blockIdx.y];
    const int side = blockIdx.z, Ks = side ? t.Ka : t.Kb;
    const int p = blockIdx.x * kJBlock + threadIdx.x;   // row 0: the prior; above: sorted slot p - 1; else trial p - 1
    if (p >= Ks) return;
    const int l = t.label;
    const int64_t n = counts[2 * l + side];
    const size_t row0 = side ? (size_t)t.Kb : 0;
    auto put = [&](int64_t row, double wv, double m, double s) {   // (SCOTT: no task supplies W)
        const size_t k = row0 + (size_t)row;
        t.mu[k * t.D + t.d] = m;
        t.sig[k * t.D + t.d] = s;
        if (t.flags & 2) t.W[k] = wv;
    };
    const double pmu = specs[l].prior_mu;
    if (n != Ks - 1 || (side == 0 && n > tpe_rt::kBuildMaxLF)) {   // not the group's trials: rows that fold, flagged
        atomicOr(flags + t.group, kJFlagCount);
        put(p, 1.0 / (double)Ks, t.upper > 0 ? 0.0 : pmu, 1.0);
        return;
    }
    const int64_t off = p_off[l];
    const double* __restrict__ bv = below_val + (size_t)l * tpe_rt::kBuildMaxLF;
    if (t.upper > 0) {   // the observed category, in observation order on both sides
        double c = 0.0;
        if (p > 0) {
            c = side ? keys[off + p - 1] : bv[p - 1];
            if (!(c >= 0.0 && c < (double)t.upper && c == floor(c))) {
                atomicOr(flags + t.group, kJFlagCat);
                c = 0.0;   // (k_joint_fold indexes the prior with it)
            }
        }
        put(p, 0.0, c, 1.0);
        return;
    }
    const double* __restrict__ sk = keys + off;
    const bool sup = (t.flags & 1) != 0;
    // the row of sorted slot q of the above list: its trial r, from the supplied order or the build's rank map
    auto above_row = [&](int64_t q) -> int64_t {
        const int32_t r = sup ? order[order_off[l] + q] : idx[off + q];
        if (r < 0 || r >= n) {
            atomicOr(flags + t.group, kJFlagCount);
            return -1;
        }
        return (int64_t)r + 1;
    };
    if constexpr (SCOTT) {
        const double psig = specs[l].prior_sigma;
        if (p == 0) {
            put(0, 0.0, pmu, psig);
            return;
        }
        const double lo = psig / fmin(100.0, 1.0 + (double)Ks);
        const double s = fmin(fmax((side ? t.fa : t.fb) * psig, lo), psig);   // np.clip (finite terms)
        if (side == 0) {
            put(p, 0.0, bv[p - 1], s);
            return;
        }
        const int64_t row = above_row(p - 1);
        if (row >= 0) put(row, 0.0, sk[p - 1], s);
    } else {
        const int64_t o = mix_off[2 * l + side];
        // the prior's slot: np.searchsorted(sorted, prior_mu), side='left' (k_parzen)
        int64_t pos = 0;
        if (n == 1) {
            pos = pmu < (side ? sk[0] : bv[0]) ? 0 : 1;
        } else if (side == 0) {
            for (int64_t j = 0; j < n; ++j) pos += bv[j] < pmu ? 1 : 0;
        } else {
            int64_t lo = 0, hi = n;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (sk[mid] < pmu) lo = mid + 1; else hi = mid;
            }
            pos = lo;
        }
        if (p == 0) {
            put(0, w[o + pos], pmu, sigma[o + pos]);
            return;
        }
        if (side == 0) {   // trial p - 1: its rank among the below values, ties by position
            const int64_t ti = p - 1;
            const double v = bv[ti];
            int64_t rank = 0;
            bool tie = v != v;
            for (int64_t j = 0; j < n; ++j) {
                const double vj = bv[j];
                rank += (vj < v || (vj == v && j < ti)) ? 1 : 0;
                tie |= j != ti && vj == v;
            }
            if (tie) atomicOr(flags + t.group, kJFlagTie);
            const int64_t j = rank < pos ? rank : rank + 1;
            put(p, w[o + j], v, sigma[o + j]);
            return;
        }
        const int64_t q = p - 1;   // sorted slot q
        const double v = sk[q];
        if (v != v || (!sup && q > 0 && sk[q - 1] == v)) atomicOr(flags + t.group, kJFlagTie);
        const int64_t row = above_row(q);
        const int64_t j = q < pos ? q : q + 1;
        if (row >= 0) put(row, w[o + j], v, sigma[o + j]);
    }
}

// The build under label shards: a group's labels live on different devices.
// The columns of a call -- per group W [K], then per dimension mu [K] and
// sig [K], K = Kb + Ka -- have the same place in every device's column buffer:
// the owner of a label gathers its columns (k_joint_gather on a one-dimension
// task), every device copies in the columns it does not own, device to
// device, and k_joint_interleave writes the slot's [K][D] arrays from them.
__global__ __launch_bounds__(kJBlock) void k_joint_interleave(const double* __restrict__ cols, int32_t D, int32_t K,
                                                              double* __restrict__ W, double* __restrict__ mu,
                                                              double* __restrict__ sig) {
    const int64_t e = (int64_t)blockIdx.x * kJBlock + threadIdx.x;
    if (e >= (int64_t)K * D) return;
    const int64_t k = e / D, d = e - k * D;
    mu[e] = cols[(size_t)K * (1 + 2 * d) + k];
    sig[e] = cols[(size_t)K * (2 + 2 * d) + k];
    if (d == 0) W[k] = cols[k];
}

// The plan of a device build call.  One device (and each device of a
// replicated context) owns every dimension, and a task's destination is the
// slot's own [K][D] arrays: one phase, one synchronisation.  Under label
// shards a device owns the dimensions whose labels it holds and a task's
// destination is its column buffer: the gather phase on every device, the
// caller's barrier, then the fold phase.
struct JBuildPlan {
    bool sharded = false;
    int32_t n_groups = 0, maxK = 1;
    int32_t bw = TPE_JOINT_BW_NEIGHBOUR;
    double prior_weight = 0.0;
    std::vector<int32_t> slots;
    std::vector<uint32_t> picks;
    std::vector<int64_t> goff;
    std::vector<GInfo> gi;
    std::vector<int32_t> owner, local;    // per dimension, flat over the groups: its label's device and index there
    std::vector<int32_t> wdim;            // per group: the dimension that supplies W
    std::vector<int32_t> flags;           // per group: one device, read back with the fold errors; label shards,
                                          //   the OR over the devices (between the phases)
    // label shards only
    std::vector<size_t> base;             // per group: its first column in the buffer (doubles)
    size_t total = 0;
    std::vector<int> device;              // per context: its HIP ordinal
    std::vector<double*> cols;            // per context: its column buffer (set by the gather phase)
    std::vector<std::vector<int32_t>> dflags;   // per context: the flags its gather raised
};

tpe_ctx* jdev(tpe_ctx* c, int d) { return d == 0 ? c : c->peers[d - 1]; }

size_t jcol_mu(const JBuildPlan& P, int32_t g, int d) {
    return P.base[g] + (size_t)(P.gi[g].Kb + P.gi[g].Ka) * (1 + 2 * (size_t)d);
}

// the device's univariate build is the current one of its resident history
int joint_build_current(tpe_ctx* ctx) {
    auto& B = ctx->build;
    const int32_t L = B.n_labels;
    if (!B.hist_ready || !B.built_ok || B.built_gen != B.hist_gen || L < 1 || (int32_t)B.specs_h.size() != L ||
        (int32_t)ctx->resident.h_labels.size() != L || ctx->resident.n_labels != L ||
        (int32_t)B.ord_cur.size() != L)
        return ctx->fail(TPE_ERR_ARG, "tpe_joint_build_groups: no current build of the resident history");
    return TPE_OK;
}

// Validate a build call into its plan.  sharded: ctx is the primary of a
// label-sharded context and a label's record is its owner's; else ctx's own.
int joint_build_plan(tpe_ctx* ctx, bool sharded, int32_t n_groups, const int32_t* slots, const uint32_t* pick_streams,
                     const int64_t* group_off, const int32_t* labels, const int32_t* streams, const double* q,
                     const int32_t* upper, const double* cat_p, double prior_weight, int32_t bw, const int32_t* flags,
                     JBuildPlan& P) {
    if (n_groups < 1 || n_groups > kJMaxGroups)
        return ctx->fail(TPE_ERR_ARG, "tpe_joint_build_groups: 1 to " + std::to_string(kJMaxGroups) + " groups");
    if (!slots || !pick_streams || !group_off || !labels || !streams || !flags)
        return ctx->fail(TPE_ERR_ARG, "null pointer");
    if (bw != TPE_JOINT_BW_NEIGHBOUR && bw != TPE_JOINT_BW_SCOTT)
        return ctx->fail(TPE_ERR_ARG, "tpe_joint_build_groups_bw: bandwidth is TPE_JOINT_BW_NEIGHBOUR or "
                                      "TPE_JOINT_BW_SCOTT");
    if (bw == TPE_JOINT_BW_SCOTT && !(prior_weight > 0.0 && prior_weight < __builtin_inf()))
        return ctx->fail(TPE_ERR_ARG, "TPE_JOINT_BW_SCOTT needs a positive finite prior weight");
    const int nd = sharded ? 1 + (int)ctx->peers.size() : 1;
    int rc;
    if (!sharded) {
        if ((rc = joint_build_current(ctx))) return rc;
    } else {   // (every device's own check ran before: tpe1_joint_lsh_check)
        for (int d = 0; d < nd; ++d)
            if (jdev(ctx, d)->build.n_labels != (int32_t)ctx->lsh_ids[d].size())
                return ctx->fail(TPE_ERR_ARG, "tpe_joint_build_groups: no current build of the resident history");
    }
    const int32_t L = sharded ? ctx->lsh_L : ctx->build.n_labels;
    if (group_off[0] != 0) return ctx->fail(TPE_ERR_ARG, "group offsets start at 0");
    P.sharded = sharded;
    P.n_groups = n_groups;
    P.bw = bw;
    P.prior_weight = prior_weight;
    P.gi.assign(n_groups, GInfo{});
    std::vector<uint8_t> seen(L, 0), slot_seen(kJMaxGroups, 0);
    std::vector<JDimSpec> ds;
    size_t cat_at = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        GInfo& I = P.gi[g];
        if (slots[g] < 0 || slots[g] >= kJMaxGroups || slot_seen[slots[g]])
            return ctx->fail(TPE_ERR_ARG, "joint slots are distinct and in [0, " + std::to_string(kJMaxGroups) + ")");
        slot_seen[slots[g]] = 1;
        const int64_t a = group_off[g], b = group_off[g + 1];
        if (b - a < 1 || b - a > kJMaxD)
            return ctx->fail(TPE_ERR_ARG, "a joint group holds 1 to " + std::to_string(kJMaxD) + " dimensions");
        const int D = (int32_t)(b - a);
        ds.resize(D);
        int first = -1;   // the first dimension that is not categorical: it supplies W and the side counts
        for (int d = 0; d < D; ++d) {
            const int32_t l = labels[a + d];
            if (l < 0 || l >= L) return ctx->fail(TPE_ERR_ARG, "tpe_joint_build_groups: label index out of range");
            if (seen[l]) return ctx->fail(TPE_ERR_ARG, "tpe_joint_build_groups: a label is listed twice");
            seen[l] = 1;
            const int32_t o = sharded ? ctx->lsh_dev[l] : 0, j = sharded ? ctx->lsh_local[l] : l;
            P.owner.push_back(o);
            P.local.push_back(j);
            const tpe_ctx* x = jdev(ctx, o);
            const tpe_label_spec& s = x->build.specs_h[j];
            const int32_t C = upper ? upper[a + d] : 0;
            if ((C > 0) != (s.kind == TPE_CATEGORICAL) || (C > 0 && C != s.upper))
                return ctx->fail(TPE_ERR_ARG, "upper must be the resident label's categories, 0 for a continuous label");
            if (C <= 0 && first < 0) {   // (C < 0: the layout refuses it)
                first = d;
                I.Kb = x->resident.h_labels[j].nb;
                I.Ka = x->resident.h_labels[j].na;
            }
            // (an unbounded label's low and high are 0, as joint_prior's)
            const int32_t fl = s.flags & (TPE_HAS_LOW | TPE_HAS_HIGH);
            ds[d] = JDimSpec{fl ? s.low : 0.0, fl ? s.high : 0.0, s.prior_mu, q ? q[a + d] : 0.0,
                             fl, s.kind == TPE_LGMM1 ? 1 : 0, C, streams[a + d]};
        }
        if (first < 0) return ctx->fail(TPE_ERR_ARG, "a device-built joint group needs a label that is not categorical");
        if (I.Kb < 1 || I.Kb > kJMaxBelow || I.Ka < 1)
            return ctx->fail(TPE_ERR_ARG, "each side needs its prior component (below: at most " +
                                              std::to_string(kJMaxBelow) + ")");
        if ((rc = joint_layout(ctx, ds, cat_p ? cat_p + cat_at : nullptr, prior_weight, I))) return rc;
        cat_at += (size_t)I.ncat;
        P.maxK = std::max(P.maxK, std::max(I.Kb, I.Ka));
        P.wdim.push_back(first);
        P.base.push_back(P.total);
        P.total += (size_t)(I.Kb + I.Ka) * (1 + 2 * (size_t)D);
    }
    P.slots.assign(slots, slots + n_groups);
    P.picks.assign(pick_streams, pick_streams + n_groups);
    P.goff.assign(group_off, group_off + n_groups + 1);
    P.flags.assign(n_groups, 0);
    if (sharded) {
        for (int d = 0; d < nd; ++d) P.device.push_back(jdev(ctx, d)->device);
        P.cols.assign(nd, nullptr);
        P.dflags.assign(nd, std::vector<int32_t>(n_groups, 0));
    }
    return TPE_OK;
}

// The gather phase on device d: the slots reserved, one task per dimension
// the device owns, the gather and (TPE_JOINT_BW_SCOTT) the weight columns
// queued; G->berr holds the groups' flags, then their fold errors.  Under
// label shards the device's flags are read back and the stream synchronised:
// the other devices read these columns in the fold phase.
int joint_build_gather(tpe_ctx* x, int d, JBuildPlan& P) {
    auto& B = x->build;
    HIPCHK(x, hipSetDevice(x->device));
    JointGroups* G = jgroups(x, true);
    hipStream_t st = x->stream;
    if (P.sharded) {
        HIPCHK(x, G->bcols.reserve(P.total));
        P.cols[d] = G->bcols.p;
    }
    const bool scott = P.bw == TPE_JOINT_BW_SCOTT;
    std::vector<JGDim> tasks;
    std::vector<tpe_rt::JointWTask> wts;   // scott: the weight columns of the groups whose W dimension is here
    int rc;
    for (int32_t g = 0; g < P.n_groups; ++g) {
        const GInfo& I = P.gi[g];
        JointState* J = nullptr;
        if ((rc = joint_reserve_slot(x, G, P.slots[g], I, &J))) return rc;
        const int32_t K = I.Kb + I.Ka;
        const double fb = scott ? tpe_joint_bandwidth_factor(I.Kb - 1, I.D) : 0.0,
                     fa = scott ? tpe_joint_bandwidth_factor(I.Ka - 1, I.D) : 0.0;
        for (int dd = 0; dd < I.D; ++dd) {
            const size_t at = (size_t)P.goff[g] + dd;
            if (P.owner[at] != d) continue;
            const int32_t l = P.local[at];
            JGDim t{J->W.p, J->mu.p, J->sig.p, fb, fa, l, g, dd, I.D, I.Kb, I.Ka, I.hd[dd].upper, B.ord_cur[l] ? 1 : 0};
            if (P.sharded) {   // its columns: column 0 of 1
                t.W = G->bcols.p + P.base[g];
                t.mu = G->bcols.p + jcol_mu(P, g, dd);
                t.sig = t.mu + K;
                t.d = 0;
                t.D = 1;
            }
            if (dd == P.wdim[g]) {
                if (scott) wts.push_back(tpe_rt::JointWTask{t.W, {0, 0}, I.Kb, I.Ka});
                else t.flags |= 2;
            }
            tasks.push_back(t);
        }
    }
    HIPCHK(x, G->err.reserve(1));
    HIPCHK(x, G->berr.reserve(2 * (size_t)P.n_groups));   // flags | fold errors, per group
    HIPCHK(x, hipMemsetAsync(G->berr.p, 0, 2 * (size_t)P.n_groups * sizeof(int32_t), st));
    if (!tasks.empty()) {
        HIPCHK(x, G->gtask.reserve(tasks.size()));
        HIPCHK(x, hipMemcpyAsync(G->gtask.p, tasks.data(), tasks.size() * sizeof(JGDim), hipMemcpyHostToDevice, st));
        const dim3 grid((unsigned)((P.maxK + kJBlock - 1) / kJBlock), (unsigned)tasks.size(), 2);
        if (scott)
            hipLaunchKernelGGL(k_joint_gather<true>, grid, dim3(kJBlock), 0, st, G->gtask.p, B.specs.p, B.p_off.p,
                               B.counts.p, B.below_val.p, B.keys.p, B.idx.p, B.order_off.p, B.order.p, nullptr,
                               nullptr, nullptr, G->berr.p);
        else
            hipLaunchKernelGGL(k_joint_gather<false>, grid, dim3(kJBlock), 0, st, G->gtask.p, B.specs.p, B.p_off.p,
                               B.counts.p, B.below_val.p, B.keys.p, B.idx.p, B.order_off.p, B.order.p, B.mix_off.p,
                               B.w.p, B.sigma.p, G->berr.p);
        HIPCHK(x, hipGetLastError());
    }
    if (!wts.empty()) {   // their sums' scratch is placed here
        int64_t leaf = 0;
        for (auto& w : wts)
            for (int side = 0; side < 2; ++side) {
                w.leaf[side] = leaf;
                leaf += (side ? w.Ka : w.Kb) / 56 + 1;
            }
        HIPCHK(x, G->bleaf.reserve((size_t)leaf));
        HIPCHK(x, G->wtask.reserve(wts.size()));
        HIPCHK(x, hipMemcpyAsync(G->wtask.p, wts.data(), wts.size() * sizeof(tpe_rt::JointWTask),
                                 hipMemcpyHostToDevice, st));
        if ((rc = tpe_rt::joint_weights_launch(x, st, G->wtask.p, (int32_t)wts.size(), P.prior_weight, kJointLF,
                                               G->bleaf.p)))
            return rc;
    }
    if (!P.sharded) return TPE_OK;
    if (!tasks.empty())
        HIPCHK(x, hipMemcpyAsync(P.dflags[d].data(), G->berr.p, P.n_groups * sizeof(int32_t), hipMemcpyDeviceToHost,
                                 st));
    HIPCHK(x, hipStreamSynchronize(st));
    return TPE_OK;
}

// The fold phase on device d.  Under label shards first the columns of the
// other devices (runs of dimensions of one owner: one copy each) and the
// slot's [K][D] arrays from them, for the groups no device flagged.  Then the
// folds, the read-back of the error words and the call's synchronisation; on
// one device the flags come back with them, so a flagged group is folded and
// left unset, and they go to `flags` (label shards: null, the caller has them).
int joint_build_fold(tpe_ctx* x, int d, JBuildPlan& P, int32_t* flags) {
    HIPCHK(x, hipSetDevice(x->device));
    JointGroups* G = jgroups(x, true);
    hipStream_t st = x->stream;
    const int32_t n_groups = P.n_groups;
    int rc;
    auto fetch = [&](int from, size_t off, size_t count) -> int {
        double* dst = G->bcols.p + off;
        const double* src = P.cols[from] + off;
        if (P.device[from] == x->device)
            HIPCHK(x, hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToDevice, st));
        else
            HIPCHK(x, hipMemcpyPeerAsync(dst, x->device, src, P.device[from], count * sizeof(double), st));
        return TPE_OK;
    };
    for (int32_t g = 0; g < n_groups; ++g) {
        if (P.flags[g]) continue;   // (label shards; one device knows no flag yet)
        const GInfo& I = P.gi[g];
        JointState* J = G->slot[P.slots[g]].get();
        if (P.sharded) {
            const size_t K = (size_t)(I.Kb + I.Ka), at = (size_t)P.goff[g];
            const int wo = P.owner[at + P.wdim[g]];
            if (wo != d && (rc = fetch(wo, P.base[g], K))) return rc;
            for (int dd = 0; dd < I.D;) {
                const int o = P.owner[at + dd];
                int e = dd + 1;
                while (e < I.D && P.owner[at + e] == o) ++e;
                if (o != d && (rc = fetch(o, jcol_mu(P, g, dd), 2 * K * (size_t)(e - dd)))) return rc;
                dd = e;
            }
            hipLaunchKernelGGL(k_joint_interleave, dim3((unsigned)((K * I.D + kJBlock - 1) / kJBlock)), dim3(kJBlock),
                               0, st, G->bcols.p + P.base[g], I.D, (int32_t)K, J->W.p, J->mu.p, J->sig.p);
            HIPCHK(x, hipGetLastError());
        }
        if ((rc = joint_upload_layout(x, J, I))) return rc;
        if ((rc = joint_fold_group(x, J, I, P.prior_weight, G->berr.p + n_groups + g))) return rc;
    }
    std::vector<int32_t> eh(2 * (size_t)n_groups);
    HIPCHK(x, hipMemcpyAsync(eh.data(), G->berr.p, eh.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(x, hipStreamSynchronize(st));
    if (!P.sharded)
        for (int32_t g = 0; g < n_groups; ++g) P.flags[g] = flags[g] = eh[g];
    bool zero = false;
    for (int32_t g = 0; g < n_groups; ++g) {
        JointState* J = G->slot[P.slots[g]].get();
        joint_commit(J, P.gi[g], P.prior_weight, P.picks[g], P.flags[g], eh[n_groups + g]);
        zero |= J->ready && J->zero;
    }
    if (zero) return zero_mass(x);
    return TPE_OK;
}
}  // namespace

// tpe_joint_build_groups on a label-sharded context, in the order its caller
// runs them (tpe_ctx.h)
int tpe1_joint_lsh_check(tpe_ctx* x) {
    TPE_SETTLE(x);   // (a deferred rebuild's report: its buffers are read here)
    return joint_build_current(x);
}

int tpe1_joint_lsh_plan(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const uint32_t* pick_streams,
                        const int64_t* group_off, const int32_t* labels, const int32_t* streams, const double* q,
                        const int32_t* upper, const double* cat_p, double prior_weight, int32_t bw, int32_t* flags,
                        std::shared_ptr<void>* out) {
    auto P = std::make_shared<JBuildPlan>();
    const int rc = joint_build_plan(ctx, true, n_groups, slots, pick_streams, group_off, labels, streams, q, upper,
                                    cat_p, prior_weight, bw, flags, *P);
    if (rc) return rc;
    *out = std::static_pointer_cast<void>(P);
    return TPE_OK;
}

int tpe1_joint_lsh_gather(tpe_ctx* x, int d, void* plan) {
    return joint_build_gather(x, d, *static_cast<JBuildPlan*>(plan));
}

// between the phases, on the caller's thread: a group flagged anywhere is flagged
void tpe1_joint_lsh_flags(void* plan, int32_t* flags) {
    JBuildPlan& P = *static_cast<JBuildPlan*>(plan);
    for (int32_t g = 0; g < P.n_groups; ++g) {
        int32_t f = 0;
        for (const auto& df : P.dflags) f |= df[g];
        P.flags[g] = f;
        flags[g] = f;
    }
}

int tpe1_joint_lsh_fold(tpe_ctx* x, int d, void* plan) {
    return joint_build_fold(x, d, *static_cast<JBuildPlan*>(plan), nullptr);
}

// the set slots of a context in ascending order: their dimensions into D[], their number back
int32_t tpe1_joint_set_slots(tpe_ctx* ctx, int32_t only, int32_t* D) {
    JointGroups* G = jgroups(ctx, false);
    int32_t n = 0;
    if (!G) return 0;
    for (int j = 0; j < kJMaxGroups; ++j) {
        if (only >= 0 && j != only) continue;
        if (G->slot[j] && G->slot[j]->ready) D[n++] = G->slot[j]->D;
    }
    return n;
}

extern "C" {

// (the per-device bodies; tpe_multi.hip exports the public tpe_joint_* names)
int tpe1_joint_set_group(tpe_ctx* ctx, int32_t slot, uint32_t pick_stream, const tpe_joint_dim* dims,
                         const double* q, const int32_t* upper, const double* cat_p, double prior_weight,
                         int32_t n_dims, int32_t n_below, const double* wb, const double* mub, const double* sigb,
                         int32_t n_above, const double* wa, const double* mua, const double* siga) {
    return joint_set(ctx, slot, pick_stream, dims, q, upper, cat_p, prior_weight, n_dims, n_below, wb, mub, sigb,
                     n_above, wa, mua, siga);
}

int tpe1_joint_condition_group(tpe_ctx* ctx, int32_t src_slot, int32_t dst_slot, int32_t n_fixed,
                               const int32_t* dims, const double* values) {
    return joint_condition(ctx, src_slot, dst_slot, n_fixed, dims, values);
}

int tpe1_joint_clear_groups(tpe_ctx* ctx) {
    if (!ctx) return TPE_ERR_ARG;
    JointGroups* G = jgroups(ctx, false);
    if (!G) return TPE_OK;
    for (int j = 0; j < kJMaxGroups; ++j)
        if (G->slot[j]) G->slot[j]->ready = false;   // (buffers kept for the next posterior: no hipFree per call)
    return TPE_OK;
}

int tpe1_joint_build_groups(tpe_ctx* ctx, int32_t n_groups, const int32_t* slots, const uint32_t* pick_streams,
                            const int64_t* group_off, const int32_t* labels, const int32_t* streams, const double* q,
                            const int32_t* upper, const double* cat_p, double prior_weight, int32_t bandwidth,
                            int32_t* flags) {
    if (!ctx) return TPE_ERR_ARG;
    TPE_SETTLE(ctx);   // (a deferred rebuild's report: its buffers are read here)
    JBuildPlan P;
    int rc = joint_build_plan(ctx, false, n_groups, slots, pick_streams, group_off, labels, streams, q, upper, cat_p,
                              prior_weight, bandwidth, flags, P);
    if (rc) return rc;
    if ((rc = joint_build_gather(ctx, 0, P))) return rc;
    return joint_build_fold(ctx, 0, P, flags);
}

// (host arithmetic only: posterior.joint_bandwidth_factor is the same operations in the same order)
double tpe_joint_bandwidth_factor(int32_t n, int32_t D) {
    if (n <= 1) return 0.2;
    return 0.2 * std::pow((double)n, -1.0 / (double)(D + 4));
}

int tpe1_joint_get_group(tpe_ctx* ctx, int32_t slot, int32_t side, double* w, double* mu, double* sigma, int32_t cap,
                         int32_t* n_components, int32_t* n_dims) {
    if (!ctx) return TPE_ERR_ARG;
    if (slot < 0 || slot >= kJMaxGroups || side < 0 || side > 1)
        return ctx->fail(TPE_ERR_ARG, "tpe_joint_get_group: slot in [0, " + std::to_string(kJMaxGroups) +
                                          "), side 0 (below) or 1 (above)");
    JointGroups* G = jgroups(ctx, false);
    JointState* J = G ? G->slot[slot].get() : nullptr;
    if (!J || !J->ready) return ctx->fail(TPE_ERR_ARG, "tpe_joint_get_group: no joint posterior set");
    const int32_t K = side ? J->Ka : J->Kb, D = J->D;
    if (n_components) *n_components = K;
    if (n_dims) *n_dims = D;
    const size_t m = (size_t)std::min(K, std::max(cap, 0)), r0 = side ? (size_t)J->Kb : 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (m > 0) {
        if (w) HIPCHK(ctx, hipMemcpy(w, J->W.p + r0, m * sizeof(double), hipMemcpyDeviceToHost));
        if (mu) HIPCHK(ctx, hipMemcpy(mu, J->mu.p + r0 * D, m * D * sizeof(double), hipMemcpyDeviceToHost));
        if (sigma) HIPCHK(ctx, hipMemcpy(sigma, J->sig.p + r0 * D, m * D * sizeof(double), hipMemcpyDeviceToHost));
    }
    return TPE_OK;
}

int tpe1_joint_draw_group(tpe_ctx* ctx, int32_t slot, uint64_t seed, uint32_t round, int64_t n, int64_t cand_offset,
                          double* values, int32_t* comp) {
    if (!ctx) return TPE_ERR_ARG;
    JointGroups* G = nullptr;
    JointState* J = nullptr;
    int rc = joint_ready(ctx, slot, &G, &J, "tpe_joint_draw_group");
    if (rc) return rc;
    if (!values || !comp) return ctx->fail(TPE_ERR_ARG, "null pointer");
    if ((rc = check_range(ctx, n, cand_offset))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, G->vals.reserve((size_t)n * J->D));
    HIPCHK(ctx, G->comp.reserve(n));
    HIPCHK(ctx, hipMemsetAsync(G->err.p, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_joint_draw, dim3((unsigned)((n + kJBlock - 1) / kJBlock)), dim3(kJBlock), 0, ctx->stream,
                       J->jp(), n, cand_offset, seed, round, G->vals.p, G->comp.p, G->err.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(values, G->vals.p, (size_t)n * J->D * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(comp, G->comp.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return read_err(ctx, G);
}

int tpe1_joint_score_group(tpe_ctx* ctx, int32_t slot, const double* values, int64_t n, double* ll, double* lg) {
    if (!ctx) return TPE_ERR_ARG;
    JointGroups* G = nullptr;
    JointState* J = nullptr;
    int rc = joint_ready(ctx, slot, &G, &J, "tpe_joint_score_group");
    if (rc) return rc;
    if (!values || !ll || !lg) return ctx->fail(TPE_ERR_ARG, "null pointer");
    if ((rc = check_range(ctx, n, 0))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, G->vals.reserve((size_t)n * J->D));
    HIPCHK(ctx, hipMemcpyAsync(G->vals.p, values, (size_t)n * J->D * sizeof(double), hipMemcpyHostToDevice,
                               ctx->stream));
    int32_t nparts = 0;
    if ((rc = launch_round(ctx, G, J, false, n, 0, 0, 0, true, &nparts, G->err.p))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ll, G->ll.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(lg, G->lg.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TPE_OK;
}

// tpe1_joint_score_group on configurations already on the device (d_values[n D],
// complete on the context's stream): the round is queued, nothing is waited
// for, and *d_ll / *d_lg are the slot scratch that will hold the lpdfs -- valid
// until the next joint call on the context (tpe_pool.hip copies them out on the
// same stream before it scores its next group)
int tpe1_joint_score_device(tpe_ctx* ctx, int32_t slot, const double* d_values, int64_t n, double** d_ll,
                            double** d_lg) {
    if (!ctx) return TPE_ERR_ARG;
    JointGroups* G = nullptr;
    JointState* J = nullptr;
    int rc = joint_ready(ctx, slot, &G, &J, "tpe_pool_rank");
    if (rc) return rc;
    if (!d_values || !d_ll || !d_lg) return ctx->fail(TPE_ERR_ARG, "null pointer");
    if ((rc = check_range(ctx, n, 0))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t nparts = 0;
    if ((rc = launch_round(ctx, G, J, false, n, 0, 0, 0, true, &nparts, G->err.p, nullptr, 0, d_values))) return rc;
    *d_ll = G->ll.p;
    *d_lg = G->lg.p;
    return TPE_OK;
}

// candidates [cand_offset, cand_offset + n_candidates) of the round (a shard
// of a multi-device round; the whole round: offset 0); *index is global
int tpe1_joint_suggest_group(tpe_ctx* ctx, int32_t slot, uint64_t seed, uint32_t round, int64_t n_candidates,
                             int64_t cand_offset, double* values, int64_t* index, double* ll, double* lg) {
    if (!ctx) return TPE_ERR_ARG;
    JointGroups* G = nullptr;
    JointState* J = nullptr;
    int rc = joint_ready(ctx, slot, &G, &J, "tpe_joint_suggest_group");
    if (rc) return rc;
    if (!values || !index || !ll || !lg) return ctx->fail(TPE_ERR_ARG, "null pointer");
    if ((rc = check_range(ctx, n_candidates, cand_offset))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, G->res.reserve(3 + J->D));
    HIPCHK(ctx, hipMemsetAsync(G->err.p, 0, sizeof(int32_t), ctx->stream));
    int32_t nparts = 0;
    if (ctx->opt.timing) HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = launch_round(ctx, G, J, true, n_candidates, cand_offset, seed, round, false, &nparts, G->err.p)))
        return rc;
    hipLaunchKernelGGL(k_joint_best, dim3(1), dim3(kJBlock), 0, ctx->stream, J->jp(), G->partials.p, nparts,
                       cand_offset, seed, round, 1, G->res.p);
    HIPCHK(ctx, hipGetLastError());
    if (ctx->opt.timing) HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    std::vector<double> h(3 + J->D);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), G->res.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = read_err(ctx, G))) return rc;
    if (ctx->opt.timing) {   // the round's device time (tpe_last_timing: both figures)
        HIPCHK(ctx, hipEventElapsedTime(&ctx->stats.round_ms, ctx->ev0, ctx->ev1));
        ctx->stats.score_ms = ctx->stats.round_ms;
    }
    *ll = h[0];
    *lg = h[1];
    *index = (int64_t)h[2];
    for (int d = 0; d < J->D; ++d) values[d] = h[3 + d];
    return TPE_OK;
}

// Every set slot's rounds in packed launches: per slot, chunks of whole
// rounds whose flat candidate count stays within the cap -- one k_joint_round
// (+ k_joint_merge) and one k_joint_best_cells each; a round beyond the cap
// runs alone as tpe_joint_suggest_group runs it.  The result rows of all slots and,
// in front of them, the error word are one device buffer: one copy back, one
// synchronisation.  Candidates [cand_offset, cand_offset + n_candidates) of
// every round (a shard of a multi-device call; the whole rounds: offset 0);
// the indices are global.
int tpe1_joint_suggest_batch(tpe_ctx* ctx, uint64_t seed, const uint32_t* rounds, int32_t n_rounds,
                             int64_t n_candidates, int64_t cand_offset, double* values, int64_t* index, double* ll,
                             double* lg) {
    if (!ctx) return TPE_ERR_ARG;
    if (!rounds || !values || !index || !ll || !lg) return ctx->fail(TPE_ERR_ARG, "null pointer");
    if (n_rounds < 1) return ctx->fail(TPE_ERR_ARG, "the number of rounds must be positive");
    int rc = check_range(ctx, n_candidates, cand_offset);
    if (rc) return rc;
    JointGroups* G = jgroups(ctx, false);
    std::vector<JointState*> set;
    if (G)
        for (int j = 0; j < kJMaxGroups; ++j)
            if (G->slot[j] && G->slot[j]->ready) set.push_back(G->slot[j].get());
    if (set.empty()) return ctx->fail(TPE_ERR_ARG, "tpe_joint_suggest_batch: no joint posterior set");
    size_t rows = 0, sumD = 0;
    for (JointState* J : set) {
        if (J->zero) return zero_mass(ctx);
        rows += 3 + J->D;
        sumD += J->D;
    }
    const int64_t R = n_rounds, n = n_candidates;
    const int64_t cap = ctx->opt.joint_flat_cap > 0 ? ctx->opt.joint_flat_cap : kJFlatCap;
    const int64_t per = n <= cap ? std::min<int64_t>(R, cap / n) : 0;   // rounds of a packed chunk
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t total = 1 + (size_t)R * rows;
    HIPCHK(ctx, G->bres.reserve(total));
    HIPCHK(ctx, G->rounds.reserve(R));
    if (per) {
        HIPCHK(ctx, G->ll.reserve(per * n));
        HIPCHK(ctx, G->lg.reserve(per * n));
    }
    int32_t* err = reinterpret_cast<int32_t*>(G->bres.p);
    HIPCHK(ctx, hipMemsetAsync(G->bres.p, 0, sizeof(double), st));
    HIPCHK(ctx, hipMemcpyAsync(G->rounds.p, rounds, R * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (ctx->opt.timing) HIPCHK(ctx, hipEventRecord(ctx->ev0, st));
    double* row0 = G->bres.p + 1;
    for (JointState* J : set) {
        const size_t w = 3 + J->D;
        int32_t nparts = 0;
        if (per) {
            for (int64_t r0 = 0; r0 < R; r0 += per) {
                const int64_t rc_n = std::min(per, R - r0);
                if ((rc = launch_round(ctx, G, J, true, rc_n * n, cand_offset, seed, 0, true, &nparts, err,
                                       G->rounds.p + r0, (uint32_t)n)))
                    return rc;
                hipLaunchKernelGGL(k_joint_best_cells, dim3((unsigned)rc_n), dim3(kJBlock), 0, st, J->jp(), G->ll.p,
                                   G->lg.p, G->rounds.p + r0, (uint32_t)n, cand_offset, seed, row0 + r0 * w);
                HIPCHK(ctx, hipGetLastError());
            }
        } else {
            for (int64_t r = 0; r < R; ++r) {
                if ((rc = launch_round(ctx, G, J, true, n, cand_offset, seed, rounds[r], false, &nparts, err)))
                    return rc;
                hipLaunchKernelGGL(k_joint_best, dim3(1), dim3(kJBlock), 0, st, J->jp(), G->partials.p, nparts,
                                   cand_offset, seed, rounds[r], 1, row0 + r * w);
                HIPCHK(ctx, hipGetLastError());
            }
        }
        row0 += (size_t)R * w;
    }
    if (ctx->opt.timing) HIPCHK(ctx, hipEventRecord(ctx->ev1, st));
    G->hres.resize(total);
    HIPCHK(ctx, hipMemcpyAsync(G->hres.data(), G->bres.p, total * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    int32_t e = 0;
    std::memcpy(&e, G->hres.data(), sizeof(e));
    if (e & 1) return not_reached(ctx);
    if (ctx->opt.timing) {
        HIPCHK(ctx, hipEventElapsedTime(&ctx->stats.round_ms, ctx->ev0, ctx->ev1));
        ctx->stats.score_ms = ctx->stats.round_ms;
    }
    const size_t ns = set.size();
    const double* h = G->hres.data() + 1;
    size_t doff = 0;
    for (size_t si = 0; si < ns; ++si) {
        const int D = set[si]->D;
        for (int64_t r = 0; r < R; ++r, h += 3 + D) {
            ll[r * ns + si] = h[0];
            lg[r * ns + si] = h[1];
            index[r * ns + si] = (int64_t)h[2];
            for (int d = 0; d < D; ++d) values[r * sumD + doff + d] = h[3 + d];
        }
        doff += D;
    }
    return TPE_OK;
}

}  // extern "C"
