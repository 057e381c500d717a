// tpe_interaction.hip -- pairwise hyperparameter interactions of one joint
// group (include/hyperopt_tpe.h, tpe_interactions; DESIGN.md section 6b,
// "Pairwise interactions").
//
// A side's joint Parzen mixture of a pair (d, e) is a sum of products, so its
// values on the G x G grid of the two labels' axes are a matrix product over
// the components:
//   u_kd(y)  = exp(-((y - mu_kd) / s_kd)^2 / 2) / (s_kd sqrt(2 pi))
//   acc[i,j] = sum_k (W_k u_kd(y_i)) u_ke(y_j)            [G x K] [K x G]
//   A        = sum_k (W_k m_kd) m_ke                      m: the mass inside the bounds
//   L[i,j]   = acc[i,j] / A                               (G[i,j]: the above side)
//   L_d[i]   = (sum_k (W_k u_kd(y_i)) m_ke) / A           (L_e[j], G_d[i], G_e[j] likewise)
// Per cell, in this order, every operation rounded on its own (no contraction),
// with om = 1 - alpha and ao = alpha om:
//   aL = alpha L;  p = aL + om G;              p == 0: both terms are 0
//   dev = (ao (L - G)) / p                     m - alpha, from the ratio: no cancellation
//   tv  = p (dev dev)
//   qi = alpha (L_d L_e);  ri = om (G_d G_e);  den = qi + ri
//   den == 0: dif = dev                        (m_ind = alpha)
//   else  mi = qi / den;  ci = ri / den        m_ind and 1 - m_ind
//         lo  = log L - log G
//         loi = (log L_d + log L_e) - (log G_d + log G_e)
//         lo or loi not finite:  dif = aL / p - mi      (one of m, m_ind is exactly 0 or 1)
//         else dl = lo - loi                   the difference of the two log-odds
//           dl <= 0: t = expm1(dl);   dif =  ((mi ci) t) / (1 + mi t)
//           dl >  0: t = expm1(-dl);  dif = -((mi ci) t) / (1 + ci t)
//   th  = p (dif dif)
//   V = (h_d h_e) sum tv,   H = (h_d h_e) sum th
//
// Layout in HBM (per context, grown on demand), Kp = K rounded up to kIntKC,
// Gp = G rounded up to kIntTile; the padding rows and columns are zeros:
//   U[side]    : double[n_dim][Kp][Gp]   u_kd(y_i), component-major
//   mass[side] : double[n_dim][Kp]
//   W[side]    : double[Kp]
//   A          : double[n_pairs][2]
//   marg, lmarg: double[n_pairs][4][Gp]  L_d, L_e, G_d, G_e and their logs
//   part       : double[n_pairs][tiles][2]
// Kernels:
//   k_int_factor  one exp per element of U, and the masses
//   k_int_norm    A per (pair, side)
//   k_int_marg    the four marginals of a pair: matrix-vector products over k
//   k_int_pair    the hot path: one workgroup per (pair, 64 x 64 tile of cells),
//                 4 waves, each a 32 x 32 sub-tile as 2 x 2 blocks of
//                 v_mfma_f64_16x16x4_f64 per side (8 accumulator quads a lane);
//                 the k loop stages chunks of kIntKC components of both factor
//                 tiles through LDS, double-buffered (W_k is folded into the d
//                 tile on its way into LDS); the below side, then the above
//                 side; the epilogue above straight from the accumulators
//   k_int_sum     per pair: its tile partials added in ascending tile order
// Every sum has a fixed order -- k ascending inside the matrix instruction
// chain, lanes by a shuffle tree, waves and tiles ascending -- and a partial
// belongs to one pair's tile, so H and V are the same bits from run to run,
// alone or among other pairs, and with the pairs in any order.
// int_mass, int_accumulate, int_terms, the tile's epilogue and the per-context buffers live in
// tpe_interaction.h, shared with tpe_interaction_mixed.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"
#include "tpe_interaction.h"

namespace {

struct IntArgs {
    IntSide side[2];
    const double *y, *h, *low, *high;   // [n_dim][n_grid], [n_dim] x3
    const int32_t* pairs;               // [n_pairs][2]
    double *A, *marg, *lmarg, *part, *out;
    double *planeL, *planeG;
    int32_t n_dim, n_grid, Gp, n_pairs;
    double alpha;
};

// grid (ceil(Kp Gp / 256), n_dim, 2)
__global__ __launch_bounds__(kIntThreads) void k_int_factor(IntArgs a) {
#pragma clang fp contract(off)
    const IntSide S = a.side[blockIdx.z];
    const int d = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * kIntThreads + threadIdx.x;
    const int64_t k = e / a.Gp;
    const int i = (int)(e - k * a.Gp);
    if (k >= S.Kp) return;
    double val = 0.0, mu = 0.0, s = 1.0;
    if (k < S.K) {
        mu = S.mu[k * a.n_dim + d];
        s = S.sig[k * a.n_dim + d];
        if (i < a.n_grid) {
            const double z = (a.y[(int64_t)d * a.n_grid + i] - mu) / s;
            val = exp(-0.5 * (z * z)) / (s * 2.5066282746310002);
        }
    }
    S.U[((int64_t)d * S.Kp + k) * a.Gp + i] = val;
    if (i == 0) {
        double m = 0.0;
        if (k < S.K) {
            const double lo = a.low[d], hi = a.high[d];
            m = (lo == lo && hi == hi) ? int_mass(mu, s, lo, hi) : 1.0;
        }
        S.mass[(int64_t)d * S.Kp + k] = m;
    }
}

// A = sum_k (W_k m_kd) m_ke: grid (n_pairs, 2); thread t sums k = t, t + 256,
// ...; the 256 sums are added ascending
__global__ __launch_bounds__(kIntThreads) void k_int_norm(IntArgs a) {
#pragma clang fp contract(off)
    const IntSide S = a.side[blockIdx.y];
    const int d = a.pairs[2 * blockIdx.x], e = a.pairs[2 * blockIdx.x + 1];
    const double* md = S.mass + (int64_t)d * S.Kp;
    const double* me = S.mass + (int64_t)e * S.Kp;
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

// The marginals: grid (n_pairs, 4, Gp / 64); vector v = 2 side + which, which
// 0: label d against the masses of e, 1: label e against those of d.  Slice q
// of a column sums k = q, q + 4, ...; the four slices are added ascending.
__global__ __launch_bounds__(kIntThreads) void k_int_marg(IntArgs a) {
#pragma clang fp contract(off)
    const int v = blockIdx.y, p = blockIdx.x;
    const IntSide S = a.side[v >> 1];
    const int d = a.pairs[2 * p + (v & 1)], o = a.pairs[2 * p + 1 - (v & 1)];
    const int q = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int i = blockIdx.z * 64 + c;
    const double* U = S.U + (int64_t)d * S.Kp * a.Gp + i;
    const double* mo = S.mass + (int64_t)o * S.Kp;
    __shared__ double ws[kIntMargSplit][64];
    double s = 0.0;
    for (int64_t k = q; k < S.K; k += kIntMargSplit) s += (S.w[k] * U[k * a.Gp]) * mo[k];
    ws[q][c] = s;
    __syncthreads();
    if (q == 0) {
        double t = ws[0][c];
#pragma unroll
        for (int r = 1; r < kIntMargSplit; ++r) t += ws[r][c];
        const double val = t / a.A[2 * p + (v >> 1)];
        const int64_t at = ((int64_t)p * 4 + v) * a.Gp + i;
        a.marg[at] = val;
        a.lmarg[at] = log(val);
    }
}

// grid (n_pairs, tile rows, tile columns)
template <bool PLANES>
__global__ __launch_bounds__(kIntThreads) void k_int_pair(IntArgs a) {
    const int p = blockIdx.x, ti = blockIdx.y, tj = blockIdx.z;
    const int d = a.pairs[2 * p], e = a.pairs[2 * p + 1];
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
        int_accumulate(S.U + (int64_t)d * S.Kp * a.Gp + i0, a.Gp, S.U + (int64_t)e * S.Kp * a.Gp + j0, a.Gp, S.w,
                       (int)(S.Kp / kIntKC), As, Bs, s ? accG : accL);
    }

    const int64_t cells = (int64_t)p * a.n_grid * a.n_grid;
    int_tile_epilogue<PLANES>(accL, accG, i0, j0, a.n_grid, a.n_grid, a.A[2 * p], a.A[2 * p + 1],
                              a.marg + (int64_t)p * 4 * a.Gp, a.lmarg + (int64_t)p * 4 * a.Gp, a.Gp, a.alpha,
                              PLANES ? a.planeL + cells : nullptr, PLANES ? a.planeG + cells : nullptr, ws,
                              a.part + 2 * (((int64_t)p * gridDim.y + ti) * gridDim.z + tj));
}

// out[p] = (V, H): from 0.0 the pair's partials in ascending tile order, then
// the cell area
__global__ __launch_bounds__(kIntThreads) void k_int_sum(IntArgs a, int32_t tiles) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * kIntThreads + threadIdx.x;
    if (p >= a.n_pairs) return;
    double v = 0.0, h = 0.0;
    for (int64_t t = 0; t < tiles; ++t) {
        v += a.part[2 * ((int64_t)p * tiles + t)];
        h += a.part[2 * ((int64_t)p * tiles + t) + 1];
    }
    const double hh = a.h[a.pairs[2 * p]] * a.h[a.pairs[2 * p + 1]];
    a.out[2 * p] = hh * v;
    a.out[2 * p + 1] = hh * h;
}

}  // namespace

extern "C" {

int tpe_interactions(tpe_ctx* ctx, int32_t n_dim, int32_t n_grid, const double* y, const double* h, const double* low,
                     const double* high, int64_t Kb, const double* wb, const double* mub, const double* sigb,
                     int64_t Ka, const double* wa, const double* mua, const double* siga, double alpha,
                     int32_t n_pairs, const int32_t* pairs, double* H, double* V, double* L, double* G) {
    if (!ctx) return TPE_ERR_ARG;
    const std::string fn = "tpe_interactions";
    if (ctx->precision != TPE_F64) return ctx->fail(TPE_ERR_ARG, fn + ": needs a TPE_F64 context");
    if (!y || !h || !low || !high || !wb || !mub || !sigb || !wa || !mua || !siga || n_pairs < 0 ||
        (n_pairs > 0 && (!pairs || !H || !V)) || (L == nullptr) != (G == nullptr))
        return ctx->fail(TPE_ERR_ARG, fn + ": null pointer or negative count");
    if (n_dim < 2) return ctx->fail(TPE_ERR_ARG, fn + ": needs at least 2 labels");
    if (n_grid < 1 || n_grid > TPE_INTERACTIONS_MAX_GRID)
        return ctx->fail(TPE_ERR_ARG, fn + ": n_grid must lie in [1, " + std::to_string(TPE_INTERACTIONS_MAX_GRID) + "]");
    if (Kb < 2 || Ka < 2) return ctx->fail(TPE_ERR_ARG, fn + ": needs the prior and at least one trial on each side");
    if (!(alpha > 0.0 && alpha < 1.0)) return ctx->fail(TPE_ERR_ARG, fn + ": alpha must lie in (0, 1)");
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t d = pairs[2 * p], e = pairs[2 * p + 1];
        if (d < 0 || d >= n_dim || e < 0 || e >= n_dim || d == e)
            return ctx->fail(TPE_ERR_ARG, fn + ": pair " + std::to_string(p) + ": two different labels in [0, n_dim)");
    }
    for (int side = 0; side < 2; ++side) {
        const double* s = side ? siga : sigb;
        const int64_t n = (side ? Ka : Kb) * n_dim;
        for (int64_t i = 0; i < n; ++i)
            if (!(s[i] > 0.0 && s[i] < HUGE_VAL)) return ctx->fail(TPE_ERR_ARG, fn + ": sigmas must be positive and finite");
    }
    if (n_pairs == 0) return TPE_OK;

    const int32_t Gp = (int32_t)int_round_up(n_grid, kIntTile), nt = Gp / kIntTile;
    const int64_t K[2] = {Kb, Ka}, Kp[2] = {int_round_up(Kb, kIntKC), int_round_up(Ka, kIntKC)};
    const double* w_in[2] = {wb, wa};
    const double* mu_in[2] = {mub, mua};
    const double* sig_in[2] = {sigb, siga};

    // (a multi-device context: its primary device)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    IntState* I = int_of(ctx);
    const int64_t n_cells = (int64_t)n_pairs * n_grid * n_grid;
    HIPCHK(ctx, I->y.reserve((size_t)n_dim * n_grid));
    HIPCHK(ctx, I->geo.reserve((size_t)3 * n_dim));
    HIPCHK(ctx, I->pairs.reserve((size_t)2 * n_pairs));
    HIPCHK(ctx, I->A.reserve((size_t)2 * n_pairs));
    HIPCHK(ctx, I->marg.reserve((size_t)n_pairs * 4 * Gp));
    HIPCHK(ctx, I->lmarg.reserve((size_t)n_pairs * 4 * Gp));
    HIPCHK(ctx, I->part.reserve((size_t)n_pairs * nt * nt * 2));
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
        HIPCHK(ctx, I->U[s].reserve((size_t)n_dim * Kp[s] * Gp));
        HIPCHK(ctx, I->mass[s].reserve((size_t)n_dim * Kp[s]));
        wpad[s].assign((size_t)Kp[s], 0.0);
        std::memcpy(wpad[s].data(), w_in[s], (size_t)K[s] * sizeof(double));
    }
    std::vector<double> geo((size_t)3 * n_dim);
    std::memcpy(geo.data(), h, n_dim * sizeof(double));
    std::memcpy(geo.data() + n_dim, low, n_dim * sizeof(double));
    std::memcpy(geo.data() + 2 * n_dim, high, n_dim * sizeof(double));
    // (pageable sources: each copy has left its source when the call returns)
    HIPCHK(ctx, hipMemcpyAsync(I->y.p, y, (size_t)n_dim * n_grid * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(I->geo.p, geo.data(), geo.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(I->pairs.p, pairs, (size_t)2 * n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, st));
    IntArgs a{};
    for (int s = 0; s < 2; ++s) {
        HIPCHK(ctx, hipMemcpyAsync(I->w[s].p, wpad[s].data(), (size_t)Kp[s] * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(I->mu[s].p, mu_in[s], (size_t)K[s] * n_dim * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(ctx,
               hipMemcpyAsync(I->sig[s].p, sig_in[s], (size_t)K[s] * n_dim * sizeof(double), hipMemcpyHostToDevice, st));
        a.side[s] = IntSide{I->w[s].p, I->mu[s].p, I->sig[s].p, I->U[s].p, I->mass[s].p, K[s], Kp[s]};
    }
    a.y = I->y.p;
    a.h = I->geo.p;
    a.low = I->geo.p + n_dim;
    a.high = I->geo.p + 2 * n_dim;
    a.pairs = I->pairs.p;
    a.A = I->A.p;
    a.marg = I->marg.p;
    a.lmarg = I->lmarg.p;
    a.part = I->part.p;
    a.out = I->out.p;
    a.planeL = L ? I->pl.p : nullptr;
    a.planeG = L ? I->pg.p : nullptr;
    a.n_dim = n_dim;
    a.n_grid = n_grid;
    a.Gp = Gp;
    a.n_pairs = n_pairs;
    a.alpha = alpha;

    const int64_t Kmax = std::max(Kp[0], Kp[1]);
    hipLaunchKernelGGL(k_int_factor, dim3((unsigned)((Kmax * Gp + kIntThreads - 1) / kIntThreads), n_dim, 2),
                       dim3(kIntThreads), 0, st, a);
    hipLaunchKernelGGL(k_int_norm, dim3(n_pairs, 2), dim3(kIntThreads), 0, st, a);
    hipLaunchKernelGGL(k_int_marg, dim3(n_pairs, 4, nt), dim3(kIntThreads), 0, st, a);
    HIPCHK(ctx, hipGetLastError());
    I->timed = false;
    for (hipEvent_t& e : I->ev)
        if (!e) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, hipEventRecord(I->ev[0], st));
    if (L)
        hipLaunchKernelGGL(k_int_pair<true>, dim3(n_pairs, nt, nt), dim3(kIntThreads), 0, st, a);
    else
        hipLaunchKernelGGL(k_int_pair<false>, dim3(n_pairs, nt, nt), dim3(kIntThreads), 0, st, a);
    HIPCHK(ctx, hipEventRecord(I->ev[1], st));
    hipLaunchKernelGGL(k_int_sum, dim3((n_pairs + kIntThreads - 1) / kIntThreads), dim3(kIntThreads), 0, st, a,
                       nt * nt);
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

int tpe_interactions_last_pair_ms(tpe_ctx* ctx, float* ms) {
    if (!ctx || !ms) return TPE_ERR_ARG;
    IntState* I = static_cast<IntState*>(ctx->inter.get());
    if (!I || !I->timed) return ctx->fail(TPE_ERR_ARG, "tpe_interactions_last_pair_ms: no tpe_interactions call with pairs yet");
    HIPCHK(ctx, hipEventElapsedTime(ms, I->ev[0], I->ev[1]));
    return TPE_OK;
}

}  // extern "C"
