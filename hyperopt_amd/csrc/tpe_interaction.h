// tpe_interaction.h -- what the two pairwise-interaction units share
// (tpe_interaction.hip: dense labels, one grid size; tpe_interaction_mixed.hip:
// quantized and categorical axes of their own sizes): the tile constants, the
// mass inside the bounds, the MFMA accumulate of a 64 x 64 tile, the two terms
// of a cell and the per-context buffers.  DESIGN.md section 6b, "Pairwise
// interactions".
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>

#include "tpe_ctx.h"

namespace {

constexpr int kIntTile = 64;   // cells per tile edge (4 waves of 32 x 32)
constexpr int kIntKC = 16;     // components per LDS chunk
// LDS row stride in doubles: 80 * 8 B = 2.5 x 256 B, so the four component
// rows a wave reads in one ds_read_b64 start 32 banks apart
constexpr int kIntLD = 80;
constexpr int kIntThreads = 256;
constexpr int kIntMargSplit = 4;   // k slices of a marginal, combined ascending

typedef double v4d __attribute__((ext_vector_type(4)));

struct IntSide {
    const double *w, *mu, *sig;   // [Kp] (zero padded), [K][n_dim] x2
    double *U, *mass;             // the factors (component-major per label), [n_dim][Kp]
    int64_t K, Kp;
};

// 1 - Phi(x) = erfc(x / sqrt 2) / 2
__device__ __forceinline__ double int_tail(double x) { return 0.5 * erfc(x / 1.4142135623730951); }

// Phi((high - mu)/s) - Phi((low - mu)/s) from the two tails on the side of the
// mean the interval lies on
__device__ __forceinline__ double int_mass(double mu, double s, double low, double high) {
#pragma clang fp contract(off)
    const double a = (low - mu) / s, b = (high - mu) / s;
    if (a >= 0.0) return int_tail(a) - int_tail(b);
    if (b <= 0.0) return int_tail(-b) - int_tail(-a);
    return 1.0 - int_tail(-a) - int_tail(b);
}

// One side's acc += (W U_d)^T U_e over `nchunks` chunks of kIntKC components,
// for the 64 x 64 tile whose factor rows start at Ud (row stride ldd) and Ue
// (lde).  As / Bs: the two LDS buffers of each factor tile.  A chunk is 16 x
// 64 doubles per tile: a thread moves two double2 of each.
__device__ __forceinline__ void int_accumulate(const double* Ud, int ldd, const double* Ue, int lde, const double* w,
                                               int nchunks, double (*As)[kIntKC][kIntLD],
                                               double (*Bs)[kIntKC][kIntLD], v4d (&acc)[2][2]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int row[2] = {t >> 5, (t + kIntThreads) >> 5}, col = (t & 31) * 2;
    double2 ra[2], rb[2];
    double wk[2];
    auto fetch = [&](int c) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int64_t k = (int64_t)c * kIntKC + row[r];
            ra[r] = *reinterpret_cast<const double2*>(Ud + k * ldd + col);
            rb[r] = *reinterpret_cast<const double2*>(Ue + k * lde + col);
            wk[r] = w[k];
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            As[buf][row[r]][col] = wk[r] * ra[r].x;
            As[buf][row[r]][col + 1] = wk[r] * ra[r].y;
            Bs[buf][row[r]][col] = rb[r].x;
            Bs[buf][row[r]][col + 1] = rb[r].y;
        }
    };
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) fetch(c + 1);
#pragma unroll
        for (int kk = 0; kk < kIntKC; kk += 4) {
            // operand lanes: A[i = lane % 16][k = lane / 16], B[k = lane / 16][j = lane % 16]
            const int kr = kk + (lane >> 4), x = lane & 15;
            const double a0 = As[buf][kr][wr + x], a1 = As[buf][kr][wr + 16 + x];
            const double b0 = Bs[buf][kr][wc + x], b1 = Bs[buf][kr][wc + 16 + x];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        // (the other buffer was last read before the previous barrier)
        if (c + 1 < nchunks) stage(buf ^ 1);
        __syncthreads();
    }
}

// the two terms of one cell (the sequence in tpe_interaction.hip's header comment)
__device__ __forceinline__ void int_terms(double L, double G, double Ld, double Le, double Gd, double Ge, double lLd,
                                          double lLe, double lGd, double lGe, double alpha, double om, double ao,
                                          double& tv, double& th) {
#pragma clang fp contract(off)
    const double aL = alpha * L;
    const double p = aL + om * G;
    if (p == 0.0) {
        tv = th = 0.0;
        return;
    }
    const double dev = (ao * (L - G)) / p;
    tv = p * (dev * dev);
    const double qi = alpha * (Ld * Le), ri = om * (Gd * Ge), den = qi + ri;
    double dif;
    if (den == 0.0) {
        dif = dev;
    } else {
        const double mi = qi / den, ci = ri / den;
        const double lo = log(L) - log(G);
        const double loi = (lLd + lLe) - (lGd + lGe);
        const double inf = __builtin_inf();
        if (!(fabs(lo) < inf) || !(fabs(loi) < inf)) {
            dif = aL / p - mi;
        } else {
            const double dl = lo - loi;
            if (dl <= 0.0) {
                const double t = expm1(dl);
                dif = ((mi * ci) * t) / (1.0 + mi * t);
            } else {
                const double t = expm1(-dl);
                dif = -((mi * ci) * t) / (1.0 + ci * t);
            }
        }
    }
    th = p * (dif * dif);
}

// a block's (sv, sh) -> its partial: lanes by a shuffle tree, waves ascending
__device__ __forceinline__ void int_block_partial(double sv, double sh, double (*ws)[kIntThreads / 64], double* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sv += __shfl_down(sv, off, 64);
        sh += __shfl_down(sh, off, 64);
    }
    if (lane == 0) {
        ws[0][wave] = sv;
        ws[1][wave] = sh;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = ws[0][0], h = ws[1][0];
#pragma unroll
        for (int w = 1; w < kIntThreads / 64; ++w) {
            v += ws[0][w];
            h += ws[1][w];
        }
        part[0] = v;
        part[1] = h;
    }
}

// The epilogue of a 64 x 64 tile at (i0, j0) of a pair whose axes have Gd and
// Ge cells, straight from the accumulators: the two terms of every cell, the
// planes at plane[i Ge + j], the block's partial.  mg / lg: the pair's four
// marginals L_d L_e G_d G_e and their logs, ld apart.
// accumulator lanes: register r of a block holds D[i = 4 r + lane / 16][j = lane % 16] (settled by the plane
// tests at n_grid 15 .. 17: with 4 (lane / 16) + r the rows of a block come out permuted)
template <bool PLANES>
__device__ __forceinline__ void int_tile_epilogue(const v4d (&accL)[2][2], const v4d (&accG)[2][2], int i0, int j0,
                                                  int Gd, int Ge, double Ab, double Aa, const double* mg,
                                                  const double* lg, int64_t ld, double alpha, double* planeL,
                                                  double* planeG, double (*ws)[kIntThreads / 64], double* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const double om = 1.0 - alpha, ao = alpha * om;
    double sv = 0.0, sh = 0.0;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const int j = j0 + wc + bj * 16 + (lane & 15);
            const double Le = mg[ld + j], Ge_ = mg[3 * ld + j], lLe = lg[ld + j], lGe = lg[3 * ld + j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + wr + bi * 16 + 4 * r + (lane >> 4);
                if (i < Gd && j < Ge) {
                    const double L = accL[bi][bj][r] / Ab, G = accG[bi][bj][r] / Aa;
                    double tv, th;
                    int_terms(L, G, mg[i], Le, mg[2 * ld + i], Ge_, lg[i], lLe, lg[2 * ld + i], lGe, alpha, om, ao, tv,
                              th);
                    sv += tv;
                    sh += th;
                    if (PLANES) {
                        const int64_t at = (int64_t)i * Ge + j;
                        planeL[at] = L;
                        planeG[at] = G;
                    }
                }
            }
        }
    }
    int_block_partial(sv, sh, ws, part);
}

// The per-context buffers of both entry points (grown on demand).  rec: the
// mixed call's axis and pair records; its cell points and priors go in y, geo.
struct IntState {
    tpe_rt::DevBuf<double> y, geo, w[2], mu[2], sig[2], U[2], mass[2], A, marg, lmarg, part, out, pl, pg;
    tpe_rt::DevBuf<int32_t> pairs;
    tpe_rt::DevBuf<unsigned char> rec;
    tpe_rt::PinVec<double> out_h;
    hipEvent_t ev[2] = {};   // the bracket of the last call's pair kernels (tpe_interactions_last_pair_ms)
    bool timed = false;
    ~IntState() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

inline IntState* int_of(tpe_ctx* ctx) {
    if (!ctx->inter)
        ctx->inter = std::shared_ptr<void>(new IntState(), [](void* q) { delete static_cast<IntState*>(q); });
    return static_cast<IntState*>(ctx->inter.get());
}

inline int64_t int_round_up(int64_t n, int64_t to) { return (n + to - 1) / to * to; }

}  // namespace
