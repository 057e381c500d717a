// tpe_interaction_mixed.hip -- pairwise interactions of one joint group whose
// labels may be quantized or categorical (include/hyperopt_tpe.h,
// tpe_interactions_mixed; DESIGN.md section 6b, "Pairwise interactions").
//
// The sums are tpe_interaction.hip's: per side acc[i,j] = sum_k (W_k u_kd(i))
// u_ke(j), A, the four marginals, int_terms per cell.  What differs is the
// axis of a label -- its own number of cells G_d and measure -- and the
// factor u_kd(i) of cell i:
//   dense        exp(-((y_i - mu)/s)^2 / 2) / (s sqrt(2 pi))       m_kd: mass inside the bounds
//   quantized    the mass of [lb, ub] = the rounding interval of x_i with the
//                step merge q (quant_bounds' clips and logs), from the tails
//                on the side of the mean (jmass)                    m_kd: the same
//   categorical  k = 0: p[i];  k >= 1: ([i == o_k] + a p[i]) / (1 + a),
//                a = C pw / K                                       m_kd = 1
//
// Layout in HBM: Kp = K rounded up to 16; Gp_d = 16 for a narrow axis (G_d <=
// 16), else G_d rounded up to 64; U[side] holds label d's [Kp][Gp_d] block at
// Kp * (Gp_0 + .. + Gp_{d-1}), component-major, padding zeros.  marg / lmarg:
// [n_pairs][4][Gpm], Gpm the largest Gp; part: [n_pairs][maxT][2].
// Kernels:
//   k_mix_factor  one element of U a thread, a branch per axis kind; the masses
//   k_mix_norm, k_mix_marg   tpe_interaction.hip's, over per-label strides
//   k_mix_wide    wide x wide pairs: the 64 x 64 tile design of k_int_pair (the
//                 shared int_accumulate and int_tile_epilogue) over the two
//                 axes' own G and Gp -- a
//                 dense x dense pair runs the operations of k_int_pair in its
//                 order: the same bits
//   k_mix_narrow<NB>  a narrow row axis against NB blocks of 16 columns (4: a
//                 64-column tile of a wide axis; 1: a narrow axis).  No LDS in
//                 the k loop: U is component-major and both paddings are
//                 multiples of 16, so lane l's A operand U_r[k0 + l / 16][l % 16]
//                 is element l of a contiguous 512 B and its B operands are 128 B
//                 row segments -- the MFMA operand layout as it lies in memory.
//                 Wave w takes the chunks of 16 components w, w + 4, ...; W_k is
//                 multiplied into the A operand in registers; each wave holds the
//                 whole tile (NB accumulator quads a side); the four waves'
//                 accumulators meet once in LDS and are added in ascending wave
//                 order, a side at a time, each wave taking a quarter of the
//                 tile's cells into the epilogue.
//   k_mix_sum     per pair: its partials in ascending tile order, then the area
// Every sum has a fixed order and a partial belongs to one pair's tile: H and V
// are the same bits from run to run, alone or among others, in any order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"
#include "tpe_interaction.h"

namespace {

constexpr int kMixNarrow = 16;   // cells of a narrow axis: one MFMA operand
constexpr double kMixEps = 1e-12;   // the reference's EPS under the log of an interval end

struct MixAxis {
    int32_t kind, G, Gp, log, upper, pad;
    int64_t x_off, p_off, u_off;   // into x, cat_p; Gp_0 + .. + Gp_{d-1}
    double measure, low, high, step;
};

struct MixPair {
    int32_t d, e;        // the caller's orientation: planes [G_d][G_e], marginals L_d L_e G_d G_e
    int32_t r, c;        // the row and the column label of the kernel (r != d: swapped)
    int32_t ntj, tiles;  // tile columns, tiles of the pair
    int64_t plane;       // offset of its planes
};

struct MixArgs {
    IntSide side[2];
    const MixAxis* ax;
    const MixPair* pairs;
    const int32_t* list;   // the pairs of this launch's shape
    const double *x, *catp;
    double *A, *marg, *lmarg, *part, *out, *planeL, *planeG;
    int32_t n_dim, Gpm, maxT, n_pairs;
    double alpha, pw;
};

// Phi(zu sqrt 2) - Phi(zl sqrt 2) from the side of the mean the interval lies
// on (tpe_joint.hip's jmass)
__device__ __forceinline__ double mix_mass(double zl, double zu) {
#pragma clang fp contract(off)
    if (!(zu > zl)) return 0.0;
    if (zl >= 0.0 || zu <= 0.0) {
        const double a = zl >= 0.0 ? zl : -zu, b = zl >= 0.0 ? zu : -zl;
        return 0.5 * (erfc(a) - erfc(b));
    }
    return 0.5 * (erf(zu) + erf(-zl));
}

// grid (ceil(Kp Gpm / 256), n_dim, 2)
__global__ __launch_bounds__(kIntThreads) void k_mix_factor(MixArgs a) {
#pragma clang fp contract(off)
    const IntSide S = a.side[blockIdx.z];
    const int d = blockIdx.y;
    const MixAxis X = a.ax[d];
    const int64_t el = (int64_t)blockIdx.x * kIntThreads + threadIdx.x;
    const int64_t k = el / X.Gp;
    const int i = (int)(el - k * X.Gp);
    if (k >= S.Kp) return;
    double val = 0.0, mu = 0.0, s = 1.0;
    if (k < S.K) {
        mu = S.mu[k * a.n_dim + d];
        s = S.sig[k * a.n_dim + d];
        if (i < X.G) {
            if (X.kind == TPE_AXIS_DENSE) {
                const double z = (a.x[X.x_off + i] - mu) / s;
                val = exp(-0.5 * (z * z)) / (s * 2.5066282746310002);
            } else if (X.kind == TPE_AXIS_QUANTIZED) {
                const double x = a.x[X.x_off + i], half = X.step / 2.0;
                double ub = x + half, lb = x - half;
                const bool bounded = X.low == X.low && X.high == X.high;
                if (!X.log) {
                    if (bounded) {
                        ub = ub < X.high ? ub : X.high;
                        lb = lb > X.low ? lb : X.low;
                    }
                } else {
                    if (bounded) {
                        const double eh = exp(X.high), el2 = exp(X.low);
                        ub = ub < eh ? ub : eh;
                        lb = lb > el2 ? lb : el2;
                    }
                    lb = lb > 0.0 ? lb : 0.0;
                    ub = log(ub > kMixEps ? ub : kMixEps);
                    lb = log(lb > kMixEps ? lb : kMixEps);
                }
                const double r2 = s * 1.4142135623730951;
                val = mix_mass((lb - mu) / r2, (ub - mu) / r2);
            } else {
                const double p = a.catp[X.p_off + i];
                if (k == 0) {
                    val = p;
                } else {
                    const double as = ((double)X.upper * a.pw) / (double)S.K;
                    val = (((double)i == mu ? 1.0 : 0.0) + as * p) / (1.0 + as);
                }
            }
        }
    }
    S.U[(S.Kp * X.u_off + k * X.Gp) + i] = val;
    if (i == 0) {
        double m = 0.0;
        if (k < S.K) {
            const bool bounded = X.low == X.low && X.high == X.high;
            m = (X.kind != TPE_AXIS_CATEGORICAL && bounded) ? int_mass(mu, s, X.low, X.high) : 1.0;
        }
        S.mass[(int64_t)d * S.Kp + k] = m;
    }
}

// A = sum_k (W_k m_kd) m_ke: grid (n_pairs, 2); thread t sums k = t, t + 256,
// ...; the 256 sums are added ascending
__global__ __launch_bounds__(kIntThreads) void k_mix_norm(MixArgs a) {
#pragma clang fp contract(off)
    const IntSide S = a.side[blockIdx.y];
    const MixPair P = a.pairs[blockIdx.x];
    const double* md = S.mass + (int64_t)P.d * S.Kp;
    const double* me = S.mass + (int64_t)P.e * S.Kp;
    __shared__ double ws[kIntThreads];
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < S.K; k += kIntThreads) s += (S.w[k] * md[k]) * me[k];
    ws[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = ws[0];
        for (int q = 1; q < kIntThreads; ++q) t += ws[q];
        a.A[2 * blockIdx.x + blockIdx.y] = t;
    }
}

// The marginals: grid (n_pairs, 4, Gpm / 64 or 1); vector v = 2 side + which,
// which 0: label d against the masses of e, 1: label e against those of d.
// Slice q of a column sums k = q, q + 4, ...; the four slices are added
// ascending.  A column past the label's own Gp is left alone.
__global__ __launch_bounds__(kIntThreads) void k_mix_marg(MixArgs a) {
#pragma clang fp contract(off)
    const int v = blockIdx.y, p = blockIdx.x;
    const IntSide S = a.side[v >> 1];
    const MixPair P = a.pairs[p];
    const int d = (v & 1) ? P.e : P.d, o = (v & 1) ? P.d : P.e;
    const MixAxis X = a.ax[d];
    const int q = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int i = blockIdx.z * 64 + c;
    const bool live = i < X.Gp;
    const double* U = S.U + S.Kp * X.u_off + i;
    const double* mo = S.mass + (int64_t)o * S.Kp;
    __shared__ double ws[kIntMargSplit][64];
    double s = 0.0;
    if (live)
        for (int64_t k = q; k < S.K; k += kIntMargSplit) s += (S.w[k] * U[k * X.Gp]) * mo[k];
    ws[q][c] = s;
    __syncthreads();
    if (q == 0 && live) {
        double t = ws[0][c];
#pragma unroll
        for (int r = 1; r < kIntMargSplit; ++r) t += ws[r][c];
        const double val = t / a.A[2 * p + (v >> 1)];
        const int64_t at = ((int64_t)p * 4 + v) * a.Gpm + i;
        a.marg[at] = val;
        a.lmarg[at] = log(val);
    }
}

// wide x wide: grid (pairs of the shape, most tile rows, most tile columns)
template <bool PLANES>
__global__ __launch_bounds__(kIntThreads) void k_mix_wide(MixArgs a) {
    const int p = a.list[blockIdx.x], ti = blockIdx.y, tj = blockIdx.z;
    const MixPair P = a.pairs[p];
    if (tj >= P.ntj || ti * P.ntj >= P.tiles) return;   // (the whole block)
    const MixAxis Xd = a.ax[P.d], Xe = a.ax[P.e];
    const int i0 = ti * kIntTile, j0 = tj * kIntTile;
    __shared__ double As[2][kIntKC][kIntLD], Bs[2][kIntKC][kIntLD];
    __shared__ double ws[2][kIntThreads / 64];
    v4d accL[2][2], accG[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) accL[bi][bj] = accG[bi][bj] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const IntSide& S = a.side[s];
        int_accumulate(S.U + S.Kp * Xd.u_off + i0, Xd.Gp, S.U + S.Kp * Xe.u_off + j0, Xe.Gp, S.w,
                       (int)(S.Kp / kIntKC), As, Bs, s ? accG : accL);
    }
    int_tile_epilogue<PLANES>(accL, accG, i0, j0, Xd.G, Xe.G, a.A[2 * p], a.A[2 * p + 1],
                              a.marg + (int64_t)p * 4 * a.Gpm, a.lmarg + (int64_t)p * 4 * a.Gpm, a.Gpm, a.alpha,
                              PLANES ? a.planeL + P.plane : nullptr, PLANES ? a.planeG + P.plane : nullptr, ws,
                              a.part + 2 * ((int64_t)p * a.maxT + ti * P.ntj + tj));
}

// One side of a narrow tile: this wave's chunks of 16 components, 4 matrix
// instructions of 4 components each a chunk and column block.
template <int NB>
__device__ __forceinline__ void mix_narrow_accumulate(const IntSide& S, const double* Ur, const double* Uc, int ldc,
                                                      v4d (&acc)[NB]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunks = (int)(S.Kp / kIntKC);
    const int kq = lane >> 4, x = lane & 15;
    for (int c = wave; c < nchunks; c += kIntThreads / 64) {
#pragma unroll
        for (int kk = 0; kk < kIntKC; kk += 4) {
            // operand lanes: A[i = lane % 16][k = lane / 16], B[k = lane / 16][j = lane % 16]
            const int64_t k = (int64_t)c * kIntKC + kk + kq;
            const double av = S.w[k] * Ur[k * kMixNarrow + x];
            const double* b = Uc + k * ldc + x;
#pragma unroll
            for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[16 * n], acc[n], 0, 0, 0);
        }
    }
}

// The four waves' accumulators of one side through LDS; out: this wave's NB
// (block, register) items t = wave NB + q -- block t / 4, register t % 4 --
// added in ascending wave order.  Ends on a barrier: red is free again.
template <int NB>
__device__ __forceinline__ void mix_narrow_combine(const v4d (&acc)[NB], double (*red)[NB * 4][64], double (&out)[NB]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][n * 4 + r][lane] = acc[n][r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const int t = wave * NB + q;
        double s = red[0][t][lane];
#pragma unroll
        for (int w = 1; w < kIntThreads / 64; ++w) s += red[w][t][lane];
        out[q] = s;
    }
    __syncthreads();
}

// narrow x (NB blocks of 16 columns): grid (pairs of the shape, most column tiles)
template <int NB, bool PLANES>
__global__ __launch_bounds__(kIntThreads) void k_mix_narrow(MixArgs a) {
    const int p = a.list[blockIdx.x], tj = blockIdx.y;
    const MixPair P = a.pairs[p];
    if (tj >= P.tiles) return;   // (the whole block)
    const MixAxis Xr = a.ax[P.r], Xc = a.ax[P.c];
    const bool swapped = P.r != P.d;
    const int j0 = tj * 16 * NB;
    __shared__ double red[kIntThreads / 64][NB * 4][64];
    __shared__ double ws[2][kIntThreads / 64];
    double cell[2][NB];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const IntSide& S = a.side[s];
        v4d acc[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[n] = v4d{0.0, 0.0, 0.0, 0.0};
        mix_narrow_accumulate<NB>(S, S.U + S.Kp * Xr.u_off, S.U + S.Kp * Xc.u_off + j0, Xc.Gp, acc);
        mix_narrow_combine<NB>(acc, red, cell[s]);
    }
    // accumulator lanes: register r of a block holds D[i = 4 r + lane / 16][j = lane % 16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double alpha = a.alpha, om = 1.0 - alpha, ao = alpha * om;
    const double Ab = a.A[2 * p], Aa = a.A[2 * p + 1];
    // the marginal vectors of the row and of the column label: L_d L_e G_d G_e in the caller's orientation
    const double* mg = a.marg + (int64_t)p * 4 * a.Gpm;
    const double* lg = a.lmarg + (int64_t)p * 4 * a.Gpm;
    const int vr = swapped ? 1 : 0, vc = 1 - vr;
    double sv = 0.0, sh = 0.0;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        const int t = wave * NB + q, n = t >> 2, r = t & 3;
        const int i = 4 * r + (lane >> 4), j = j0 + n * 16 + (lane & 15);
        if (i < Xr.G && j < Xc.G) {
            const double L = cell[0][q] / Ab, G = cell[1][q] / Aa;
            const int64_t ri = (int64_t)vr * a.Gpm + i, cj = (int64_t)vc * a.Gpm + j, up = 2 * (int64_t)a.Gpm;
            double tv, th;
            int_terms(L, G, mg[ri], mg[cj], mg[up + ri], mg[up + cj], lg[ri], lg[cj], lg[up + ri], lg[up + cj], alpha,
                      om, ao, tv, th);
            sv += tv;
            sh += th;
            if (PLANES) {
                const int64_t at = P.plane + (swapped ? (int64_t)j * Xr.G + i : (int64_t)i * Xc.G + j);
                a.planeL[at] = L;
                a.planeG[at] = G;
            }
        }
    }
    int_block_partial(sv, sh, ws, a.part + 2 * ((int64_t)p * a.maxT + tj));
}

// out[p] = (V, H): from 0.0 the pair's partials in ascending tile order, then
// the cell area
__global__ __launch_bounds__(kIntThreads) void k_mix_sum(MixArgs a) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * kIntThreads + threadIdx.x;
    if (p >= a.n_pairs) return;
    const MixPair P = a.pairs[p];
    double v = 0.0, h = 0.0;
    for (int64_t t = 0; t < P.tiles; ++t) {
        v += a.part[2 * ((int64_t)p * a.maxT + t)];
        h += a.part[2 * ((int64_t)p * a.maxT + t) + 1];
    }
    const double hh = a.ax[P.d].measure * a.ax[P.e].measure;
    a.out[2 * p] = hh * v;
    a.out[2 * p + 1] = hh * h;
}

inline size_t pad16(size_t bytes) { return (bytes + 15) / 16 * 16; }

}  // namespace

extern "C" {

int tpe_interactions_mixed(tpe_ctx* ctx, int32_t n_dim, const tpe_interaction_axis* axes, const double* x,
                           const double* cat_p, int64_t n_cat_p, int64_t Kb, const double* wb, const double* mub,
                           const double* sigb, int64_t Ka, const double* wa, const double* mua, const double* siga,
                           double prior_weight, double alpha, int32_t n_pairs, const int32_t* pairs, double* H,
                           double* V, const int64_t* plane_off, double* L, double* G) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_interactions_mixed";
    auto finite_pos = [](double v) { return v > 0.0 && v < HUGE_VAL; };
    if (ctx->precision != TPE_F64) return ctx->fail(TPE_ERR_ARG, fn + ": needs a TPE_F64 context");
    if (!axes || !x || !wb || !mub || !sigb || !wa || !mua || !siga || n_pairs < 0 || n_cat_p < 0 ||
        (n_cat_p > 0 && !cat_p) || (n_pairs > 0 && (!pairs || !H || !V)) || (L == nullptr) != (G == nullptr) ||
        (L && n_pairs > 0 && !plane_off))
        return ctx->fail(TPE_ERR_ARG, fn + ": null pointer or negative count");
    if (n_dim < 2) return ctx->fail(TPE_ERR_ARG, fn + ": needs at least 2 labels");
    if (Kb < 2 || Ka < 2) return ctx->fail(TPE_ERR_ARG, fn + ": needs the prior and at least one trial on each side");
    if (!(alpha > 0.0 && alpha < 1.0)) return ctx->fail(TPE_ERR_ARG, fn + ": alpha must lie in (0, 1)");
    if (!finite_pos(prior_weight)) return ctx->fail(TPE_ERR_ARG, fn + ": prior_weight must be positive and finite");
    const int64_t K[2] = {Kb, Ka}, Kp[2] = {int_round_up(Kb, kIntKC), int_round_up(Ka, kIntKC)};
    const double* w_in[2] = {wb, wa};
    const double* mu_in[2] = {mub, mua};
    const double* sig_in[2] = {sigb, siga};
    std::vector<MixAxis> ax((size_t)n_dim);
    int64_t n_x = 0, gsum = 0;
    int32_t Gpm = 0;
    for (int32_t d = 0; d < n_dim; ++d) {
        const tpe_interaction_axis& t = axes[d];
        const std::string who = fn + ": axis " + std::to_string(d);
        if (t.kind != TPE_AXIS_DENSE && t.kind != TPE_AXIS_QUANTIZED && t.kind != TPE_AXIS_CATEGORICAL)
            return ctx->fail(TPE_ERR_ARG, who + ": unknown kind");
        if (t.n_cells < 1 || t.n_cells > TPE_INTERACTIONS_MAX_GRID)
            return ctx->fail(TPE_ERR_ARG, who + ": n_cells must lie in [1, " + std::to_string(TPE_INTERACTIONS_MAX_GRID) + "]");
        if (t.x_off < 0) return ctx->fail(TPE_ERR_ARG, who + ": negative offset");
        if (!finite_pos(t.measure)) return ctx->fail(TPE_ERR_ARG, who + ": the measure must be positive and finite");
        if (t.kind == TPE_AXIS_QUANTIZED && !finite_pos(t.step))
            return ctx->fail(TPE_ERR_ARG, who + ": the step must be positive and finite");
        if (t.kind == TPE_AXIS_CATEGORICAL) {
            if (t.upper != t.n_cells) return ctx->fail(TPE_ERR_ARG, who + ": upper must be the number of cells");
            if (t.p_off < 0 || t.p_off + t.upper > n_cat_p) return ctx->fail(TPE_ERR_ARG, who + ": prior outside cat_p");
            for (int32_t c = 0; c < t.upper; ++c)
                if (!finite_pos(cat_p[t.p_off + c]))
                    return ctx->fail(TPE_ERR_ARG, who + ": prior entries must be positive and finite");
            for (int s = 0; s < 2; ++s)
                for (int64_t k = 0; k < K[s]; ++k) {
                    const double o = mu_in[s][k * n_dim + d];
                    if (!(o >= 0.0 && o < (double)t.upper && o == std::floor(o)))
                        return ctx->fail(TPE_ERR_ARG, who + ": a categorical mean must be an integer in [0, upper)");
                }
        }
        const int32_t Gp = t.n_cells <= kMixNarrow ? kMixNarrow : (int32_t)int_round_up(t.n_cells, kIntTile);
        ax[d] = MixAxis{t.kind, t.n_cells, Gp, t.log != 0, t.upper, 0, t.x_off, t.p_off, gsum,
                        t.measure, t.low, t.high, t.step};
        n_x = std::max(n_x, t.x_off + t.n_cells);
        gsum += Gp;
        Gpm = std::max(Gpm, Gp);
    }
    // the pairs by shape; the narrow label of a narrow x wide pair is the row
    std::vector<MixPair> pr((size_t)n_pairs);
    std::vector<int32_t> list[3];   // wide x wide, narrow x wide, narrow x narrow
    int32_t maxT = 1, gy[3] = {1, 1, 1}, gz = 1;
    int64_t n_cells = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t d = pairs[2 * p], e = pairs[2 * p + 1];
        if (d < 0 || d >= n_dim || e < 0 || e >= n_dim || d == e)
            return ctx->fail(TPE_ERR_ARG, fn + ": pair " + std::to_string(p) + ": two different labels in [0, n_dim)");
        const bool nd = ax[d].Gp == kMixNarrow, ne = ax[e].Gp == kMixNarrow;
        MixPair& P = pr[p];
        P.d = d;
        P.e = e;
        P.r = (!nd && ne) ? e : d;
        P.c = (!nd && ne) ? d : e;
        const int shape = nd && ne ? 2 : (nd || ne) ? 1 : 0;
        P.ntj = shape == 2 ? 1 : ax[P.c].Gp / kIntTile;
        P.tiles = shape == 0 ? (ax[d].Gp / kIntTile) * P.ntj : P.ntj;
        P.plane = L ? plane_off[p] : 0;
        if (L && (P.plane < 0 || (p == 0 ? P.plane != 0 : P.plane < n_cells)))
            return ctx->fail(TPE_ERR_ARG, fn + ": plane offsets must start at 0 and leave each pair its G_d G_e cells");
        n_cells = P.plane + (int64_t)ax[d].G * ax[e].G;
        maxT = std::max(maxT, P.tiles);
        gy[shape] = std::max(gy[shape], shape == 0 ? ax[d].Gp / kIntTile : P.ntj);
        if (shape == 0) gz = std::max(gz, P.ntj);
        list[shape].push_back(p);
    }
    for (int side = 0; side < 2; ++side)
        for (int64_t k = 0; k < K[side]; ++k)
            for (int32_t d = 0; d < n_dim; ++d) {
                const double s = sig_in[side][k * n_dim + d];
                if (!finite_pos(s)) return ctx->fail(TPE_ERR_ARG, fn + ": sigmas must be positive and finite");
            }
    if (n_pairs == 0) return TPE_OK;

    // (a multi-device context: its primary device)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IntState* I = int_of(ctx);
    HIPCHK(ctx, I->y.reserve((size_t)n_x));
    HIPCHK(ctx, I->geo.reserve((size_t)std::max<int64_t>(n_cat_p, 1)));
    HIPCHK(ctx, I->A.reserve((size_t)2 * n_pairs));
    HIPCHK(ctx, I->marg.reserve((size_t)n_pairs * 4 * Gpm));
    HIPCHK(ctx, I->lmarg.reserve((size_t)n_pairs * 4 * Gpm));
    HIPCHK(ctx, I->part.reserve((size_t)n_pairs * maxT * 2));
    HIPCHK(ctx, I->out.reserve((size_t)2 * n_pairs));
    HIPCHK(ctx, I->out_h.resize((size_t)2 * n_pairs));
    if (L) {
        HIPCHK(ctx, I->pl.reserve((size_t)n_cells));
        HIPCHK(ctx, I->pg.reserve((size_t)n_cells));
    }
    std::vector<double> wpad[2];
    for (int s = 0; s < 2; ++s) {
        HIPCHK(ctx, I->w[s].reserve((size_t)Kp[s]));
        HIPCHK(ctx, I->mu[s].reserve((size_t)K[s] * n_dim));
        HIPCHK(ctx, I->sig[s].reserve((size_t)K[s] * n_dim));
        HIPCHK(ctx, I->U[s].reserve((size_t)Kp[s] * gsum));
        HIPCHK(ctx, I->mass[s].reserve((size_t)n_dim * Kp[s]));
        wpad[s].assign((size_t)Kp[s], 0.0);
        std::memcpy(wpad[s].data(), w_in[s], (size_t)K[s] * sizeof(double));
    }
    // the records in one upload: axes, pairs, the three lists
    std::vector<int32_t> lists;
    size_t list_at[3];
    for (int s = 0; s < 3; ++s) {
        list_at[s] = lists.size();
        lists.insert(lists.end(), list[s].begin(), list[s].end());
    }
    const size_t at_pr = pad16(ax.size() * sizeof(MixAxis)), at_list = at_pr + pad16(pr.size() * sizeof(MixPair)),
                 bytes = at_list + pad16(lists.size() * sizeof(int32_t));
    std::vector<unsigned char> host(bytes);
    HIPCHK(ctx, I->rec.reserve(bytes));
    std::memcpy(host.data(), ax.data(), ax.size() * sizeof(MixAxis));
    std::memcpy(host.data() + at_pr, pr.data(), pr.size() * sizeof(MixPair));
    std::memcpy(host.data() + at_list, lists.data(), lists.size() * sizeof(int32_t));
    const MixAxis* d_ax = reinterpret_cast<const MixAxis*>(I->rec.p);
    const MixPair* d_pr = reinterpret_cast<const MixPair*>(I->rec.p + at_pr);
    const int32_t* d_list = reinterpret_cast<const int32_t*>(I->rec.p + at_list);
    // (pageable sources: each copy has left its source when the call returns)
    HIPCHK(ctx, hipMemcpyAsync(I->rec.p, host.data(), bytes, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(I->y.p, x, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, st));
    if (n_cat_p > 0)
        HIPCHK(ctx, hipMemcpyAsync(I->geo.p, cat_p, (size_t)n_cat_p * sizeof(double), hipMemcpyHostToDevice, st));
    MixArgs a{};
    for (int s = 0; s < 2; ++s) {
        HIPCHK(ctx, hipMemcpyAsync(I->w[s].p, wpad[s].data(), (size_t)Kp[s] * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(I->mu[s].p, mu_in[s], (size_t)K[s] * n_dim * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(ctx,
               hipMemcpyAsync(I->sig[s].p, sig_in[s], (size_t)K[s] * n_dim * sizeof(double), hipMemcpyHostToDevice, st));
        a.side[s] = IntSide{I->w[s].p, I->mu[s].p, I->sig[s].p, I->U[s].p, I->mass[s].p, K[s], Kp[s]};
    }
    a.ax = d_ax;
    a.pairs = d_pr;
    a.x = I->y.p;
    a.catp = I->geo.p;
    a.A = I->A.p;
    a.marg = I->marg.p;
    a.lmarg = I->lmarg.p;
    a.part = I->part.p;
    a.out = I->out.p;
    a.planeL = L ? I->pl.p : nullptr;
    a.planeG = L ? I->pg.p : nullptr;
    a.n_dim = n_dim;
    a.Gpm = Gpm;
    a.maxT = maxT;
    a.n_pairs = n_pairs;
    a.alpha = alpha;
    a.pw = prior_weight;

    const int64_t Kmax = std::max(Kp[0], Kp[1]);
    hipLaunchKernelGGL(k_mix_factor, dim3((unsigned)((Kmax * Gpm + kIntThreads - 1) / kIntThreads), n_dim, 2),
                       dim3(kIntThreads), 0, st, a);
    hipLaunchKernelGGL(k_mix_norm, dim3(n_pairs, 2), dim3(kIntThreads), 0, st, a);
    hipLaunchKernelGGL(k_mix_marg, dim3(n_pairs, 4, (Gpm + 63) / 64), dim3(kIntThreads), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    I->timed = false;
    for (hipEvent_t& e : I->ev)
        if (!e) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, hipEventRecord(I->ev[0], st));
    const dim3 block(kIntThreads);
    if (!list[0].empty()) {
        a.list = d_list + list_at[0];
        const dim3 grid((unsigned)list[0].size(), gy[0], gz);
        if (L) hipLaunchKernelGGL(k_mix_wide<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_mix_wide<false>, grid, block, 0, st, a);
    }
    if (!list[1].empty()) {
        a.list = d_list + list_at[1];
        const dim3 grid((unsigned)list[1].size(), gy[1]);
        if (L) hipLaunchKernelGGL((k_mix_narrow<4, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mix_narrow<4, false>), grid, block, 0, st, a);
    }
    if (!list[2].empty()) {
        a.list = d_list + list_at[2];
        const dim3 grid((unsigned)list[2].size());
        if (L) hipLaunchKernelGGL((k_mix_narrow<1, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mix_narrow<1, false>), grid, block, 0, st, a);
    }
    HIPCHK(ctx, hipEventRecord(I->ev[1], st));
    hipLaunchKernelGGL(k_mix_sum, dim3((n_pairs + kIntThreads - 1) / kIntThreads), block, 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(I->out_h.data(), I->out.p, (size_t)2 * n_pairs * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    I->timed = true;
    for (int32_t p = 0; p < n_pairs; ++p) {
        V[p] = I->out_h[2 * p];
        H[p] = I->out_h[2 * p + 1];
    }
    // the planes (asked for by the tests) are plain copies after it
    if (L) {
        HIPCHK(ctx, hipMemcpy(L, I->pl.p, (size_t)n_cells * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(G, I->pg.p, (size_t)n_cells * sizeof(double), hipMemcpyDeviceToHost));
    }
    return TPE_OK;
}

}  // extern "C"
