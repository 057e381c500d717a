// tpe_mo.hip -- several objectives: the Pareto-compliant total order of the
// trials' objective vectors (include/hyperopt_tpe.h, tpe_mo_keys).
//
// Row i dominates row j when F[i] <= F[j] in every objective and F[i] < F[j]
// in one (IEEE comparisons: a row with a NaN is compared with nobody).
// by[i] counts the rows that dominate i, do[i] the rows i dominates; the
// order is ascending by, descending do, ascending i, and keys[i] is row i's
// position in it.
//
// Per call, in HBM (reusable buffers of the context):
//   F    : double[n][M]   the rows, as the caller holds them
//   cnt  : int32[2][n]    by, do (zeroed, then summed over the j-slices)
//   key  : uint64[n] x 2  (by, n - do, i) in b bits each, b = bit width of n
//   keys : double[n]
// Kernels
//   k_mo_pairs<M>  grid (row blocks, j-slices): a thread keeps row i in
//                  registers and reads the slice's rows j through wave-uniform
//                  loads (every lane the same address: the scalar cache, no
//                  LDS), counting both directions for its own row; one integer
//                  atomicAdd per thread, counter and slice -- integer sums are
//                  order-free, so the counts are the same bits on every run
//   k_mo_pack      (by, n - do, i) -> one key per row; a NaN row's by field is n
//   hipcub radix sort of the keys over their 3 b bits
//   k_mo_scatter   sorted position p -> keys[i] = p; NaN rows: NaN, -1, -1
//
// With constraints (tpe_mo_keys_constrained): G[n][K], c <= 0 satisfied.  The
// violation v[i] = ((0 + max(G[i][0], 0)) + max(G[i][1], 0)) + ... (additions
// only, left to right: the bits numpy gives); a row with a NaN in F[i] or G[i]
// is dead (v NaN), one with v == 0 feasible.  The order is the one above with
// the feasible rows' counts taken among feasible rows, and by = the live rows
// of smaller violation, do = 0 for an infeasible row -- past every feasible
// row's by.  Two more buffers of the context, none of them touched by the
// unconstrained call:
//   in   : double[n][M] + double[n][K]   F then G, one upload from pinned memory
//   v    : double[n]
//   cntv : int32[2][n]  the counts of the pass over v
// Kernels
//   k_moc_prep     a thread per row: the NaN flag (tested explicitly: a max
//                  swallows a NaN), v, and NaN over the row of F when the row
//                  is dead or infeasible -- in place, on the device copy
//   k_mo_pairs<M>  on that copy: the counts among feasible rows
//   k_mo_pairs<1>  on v: by = the live rows of strictly smaller violation
//   k_moc_pack     each row's fields from the pass it belongs to
//   the same sort
//   k_moc_scatter  keys[i] = p, and by, do of every live row from its key's
//                  fields (an infeasible row's: the v pass's by, 0); dead
//                  rows: NaN, -1, -1
//
// With the hypervolume tie-break (tpe_mo_keys_hv, two or three objectives):
// either pipeline above with tpe_mo_hv.hip's pairs kernel in the place of
// k_mo_pairs<M> -- it counts the rank coordinates as well -- and, behind the
// scatter, its level search, compaction and selection, which rewrite the keys
// of one level.  Buffers of the context that only this call allocates:
//   rank  : uint32[M][n]   rows j with F[j][m] < F[i][m]
//   lvl   : int32[2][n], lvl_r : uint32[M][n], flag : uint8[n]   the level
//   hdr   : int32[4]; pick : int32[64]; gain : uint64[64]
//
// With the sampled hypervolume tie-break (tpe_mo_keys_hvs, two to eight
// objectives): the same call with tpe_mo_hvs.hip's pairs kernel, level search
// and compaction; the host then reads the header (the level's size L, the
// picks q, n_f: a second synchronisation in the call), sizes the coverage matrix
// to that level and enqueues exactly q picks.  Buffers of the context that
// only this call allocates, growing only:
//   hvs_bits : uint64[S / 64][L]   hvs_pts : uint32[M][S]   hvs_lo : uint32[8]
//   hvs_cov  : uint64[S / 64]      hvs_gain : uint32[L]     hvs_pick_t : int32[64]
//
// The exclusive hypervolumes of raw rows against a reference point
// (tpe_mo_exclusive, two or three objectives; tpe_mo_exclusive4, four): the
// upload of the constrained call, k_moc_prep when constraints are given, then
// tpe_mo_hvx.hip's kernels or tpe_mo_hvx4.hip's.  Buffers of the context that
// only these calls allocate, whichever comes first (the same for both):
//   xflag : int32[n]  0 live, 1 weakly dominated within its J, 2 not valid
//   xlive : int32[n]  the live rows; xhdr : int32[2]; excl : double[n]
//
// The sampled indicator (tpe_mo_exclusive_mc, two to eight objectives): the same
// upload and k_moc_prep, then tpe_mo_hvm.hip's kernels; one read-back of the
// counts with the covered samples and the alive rows behind them.  Buffers of
// the context that only this call allocates, growing only:
//   hvm_T : uint32[n + 4][8]   hvm_alive : uint8[n + 4]    hvm_lo : double[8]
//   hvm_samp : uint64[S]       hvm_count : uint32[n + 2]
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"
#include "tpe_mo_hv.h"
#include "tpe_mo_hvm.h"
#include "tpe_mo_hvs.h"
#include "tpe_mo_hvx.h"
#include "tpe_mo_hvx4.h"

using namespace tpe_rt;

namespace {

constexpr int64_t kMoMaxRows = (int64_t)1 << 20;   // 3 x 21 bits in one key
constexpr int kMoMaxObj = 8;
constexpr int kMoMaxCon = 8;
constexpr unsigned kMoBlocks = 1024;               // workgroups wanted: 4 per CU

template <int M>
__global__ __launch_bounds__(kBlock) void k_mo_pairs(const double* __restrict__ F, int32_t n, int32_t per_slice,
                                                     int32_t* __restrict__ by, int32_t* __restrict__ dom) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    // a lane past the rows compares NaNs: every test below is false for it
    double fi[M];
#pragma unroll
    for (int m = 0; m < M; ++m) fi[m] = i < n ? F[(size_t)i * M + m] : __builtin_nan("");
    const int32_t j0 = (int32_t)blockIdx.y * per_slice;          // (uniform over the workgroup)
    const int32_t j1 = min(n, j0 + per_slice);
    int32_t n_by = 0, n_do = 0;
    // i dominates j: every fi <= fj and not every fi >= fj (some fi < fj
    // then); j dominates i the other way round.  Equal rows: both "every",
    // neither dominates.  A NaN on either side fails both "every".
    // (rows in flight: 8 doubles a row at M = 8, and the scalar registers are few)
    constexpr int kUnroll = M <= 4 ? 4 : 2;
#pragma unroll kUnroll
    for (int32_t j = j0; j < j1; ++j) {
        const double* __restrict__ fj = F + (size_t)j * M;
        bool le = true, ge = true;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const double v = fj[m];
            le &= fi[m] <= v;
            ge &= fi[m] >= v;
        }
        n_do += (le && !ge) ? 1 : 0;
        n_by += (ge && !le) ? 1 : 0;
    }
    if (i < n) {
        if (n_by) atomicAdd(by + i, n_by);
        if (n_do) atomicAdd(dom + i, n_do);
    }
}

// (by, n - do, i) in `bits` bits each; a row with a NaN: by field n, past every count
__global__ __launch_bounds__(kBlock) void k_mo_pack(const double* __restrict__ F, int32_t n, int32_t n_obj,
                                                    int32_t bits, const int32_t* __restrict__ by,
                                                    const int32_t* __restrict__ dom, uint64_t* __restrict__ key) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    bool nan = false;
    for (int m = 0; m < n_obj; ++m) {
        const double v = F[(size_t)i * n_obj + m];
        nan |= v != v;
    }
    const uint64_t b = nan ? (uint64_t)n : (uint64_t)by[i];
    const uint64_t d = (uint64_t)(n - dom[i]);
    key[i] = (b << (2 * bits)) | (d << bits) | (uint64_t)i;
}

__global__ __launch_bounds__(kBlock) void k_mo_scatter(const uint64_t* __restrict__ sorted, int32_t n, int32_t bits,
                                                       double* __restrict__ keys, int32_t* __restrict__ by,
                                                       int32_t* __restrict__ dom) {
    const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (p >= n) return;
    const uint64_t k = sorted[p];
    const int32_t i = (int32_t)(k & (((uint64_t)1 << bits) - 1));
    if ((int64_t)(k >> (2 * bits)) == n) {
        keys[i] = __builtin_nan("");
        by[i] = -1;
        dom[i] = -1;
    } else {
        keys[i] = (double)p;
    }
}

// v, and the rows of F that stay out of the dominance pass set to NaN
__global__ __launch_bounds__(kBlock) void k_moc_prep(double* __restrict__ F, const double* __restrict__ G, int32_t n,
                                                     int32_t n_obj, int32_t n_con, double* __restrict__ v) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    bool nan = false;
    for (int m = 0; m < n_obj; ++m) {
        const double f = F[(size_t)i * n_obj + m];
        nan |= f != f;
    }
    double s = 0.0;
    for (int k = 0; k < n_con; ++k) {
        const double g = G[(size_t)i * n_con + k];
        nan |= g != g;
        s = s + (g > 0.0 ? g : 0.0);   // (-inf, -0.0: zero; +inf: an ordinary value)
    }
    if (nan) s = __builtin_nan("");
    v[i] = s;
    if (!(s == 0.0))
        for (int m = 0; m < n_obj; ++m) F[(size_t)i * n_obj + m] = __builtin_nan("");
}

// feasible: (by, n - do) among feasible rows; infeasible: (live rows of smaller
// violation, n: it dominates nobody); dead: by field n
__global__ __launch_bounds__(kBlock) void k_moc_pack(const double* __restrict__ v, int32_t n, int32_t bits,
                                                     const int32_t* __restrict__ by, const int32_t* __restrict__ dom,
                                                     const int32_t* __restrict__ by_v, uint64_t* __restrict__ key) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    const double vi = v[i];
    uint64_t b, d;
    if (vi != vi) {
        b = (uint64_t)n;
        d = (uint64_t)n;
    } else if (vi == 0.0) {
        b = (uint64_t)by[i];
        d = (uint64_t)(n - dom[i]);
    } else {
        b = (uint64_t)by_v[i];
        d = (uint64_t)n;
    }
    key[i] = (b << (2 * bits)) | (d << bits) | (uint64_t)i;
}

__global__ __launch_bounds__(kBlock) void k_moc_scatter(const uint64_t* __restrict__ sorted, int32_t n, int32_t bits,
                                                        double* __restrict__ keys, int32_t* __restrict__ by,
                                                        int32_t* __restrict__ dom) {
    const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (p >= n) return;
    const uint64_t k = sorted[p];
    const uint64_t mask = ((uint64_t)1 << bits) - 1;
    const int32_t i = (int32_t)(k & mask);
    const int32_t b = (int32_t)(k >> (2 * bits));
    if (b == n) {
        keys[i] = __builtin_nan("");
        by[i] = -1;
        dom[i] = -1;
    } else {
        keys[i] = (double)p;
        by[i] = b;
        dom[i] = n - (int32_t)((k >> bits) & mask);
    }
}

struct MoState {
    DevBuf<double> F, keys;
    DevBuf<int32_t> cnt;
    DevBuf<uint64_t> key, key2;
    DevBuf<unsigned char> tmp;
    PinVec<double> keys_h;
    PinVec<int32_t> cnt_h;
    // tpe_mo_keys_constrained alone
    DevBuf<double> in, v;
    DevBuf<int32_t> cntv;
    PinVec<double> in_h, v_h;
    // tpe_mo_keys_hv alone
    DevBuf<uint32_t> rank, lvl_r;
    DevBuf<int32_t> lvl, hdr, pick;
    DevBuf<unsigned char> flag;
    DevBuf<unsigned long long> gain;
    PinVec<int32_t> pick_h;                 // hdr, then pick
    PinVec<unsigned long long> gain_h;
    // tpe_mo_keys_hvs alone
    DevBuf<uint64_t> hvs_bits, hvs_cov;
    DevBuf<uint32_t> hvs_pts, hvs_lo, hvs_gain;
    DevBuf<int32_t> hvs_pick_t;
    // tpe_mo_exclusive and tpe_mo_exclusive4 alone
    DevBuf<int32_t> xflag, xlive, xhdr;
    DevBuf<double> excl;
    PinVec<double> excl_h;
    PinVec<int32_t> xhdr_h;
    // tpe_mo_exclusive_mc alone
    DevBuf<uint32_t> hvm_T, hvm_count;
    DevBuf<unsigned char> hvm_alive;
    DevBuf<double> hvm_lo;
    DevBuf<uint64_t> hvm_samp;
    PinVec<uint32_t> hvm_count_h;
};

MoState* mo_of(tpe_ctx* ctx) {
    if (!ctx->mo) ctx->mo = std::shared_ptr<void>(new MoState(), [](void* q) { delete static_cast<MoState*>(q); });
    return static_cast<MoState*>(ctx->mo.get());
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <int M>
void launch_pairs(dim3 grid, hipStream_t st, const double* F, int32_t n, int32_t per_slice, int32_t* by,
                  int32_t* dom) {
    hipLaunchKernelGGL(k_mo_pairs<M>, grid, dim3(kBlock), 0, st, F, n, per_slice, by, dom);
}

void launch_pairs_of(int32_t n_obj, dim3 grid, hipStream_t st, const double* F, int32_t n, int32_t per_slice,
                     int32_t* by, int32_t* dom) {
    switch (n_obj) {
        case 1: launch_pairs<1>(grid, st, F, n, per_slice, by, dom); break;
        case 2: launch_pairs<2>(grid, st, F, n, per_slice, by, dom); break;
        case 3: launch_pairs<3>(grid, st, F, n, per_slice, by, dom); break;
        case 4: launch_pairs<4>(grid, st, F, n, per_slice, by, dom); break;
        case 5: launch_pairs<5>(grid, st, F, n, per_slice, by, dom); break;
        case 6: launch_pairs<6>(grid, st, F, n, per_slice, by, dom); break;
        case 7: launch_pairs<7>(grid, st, F, n, per_slice, by, dom); break;
        default: launch_pairs<8>(grid, st, F, n, per_slice, by, dom); break;
    }
}

// tpe_mo_exclusive (n_obj 2 or 3: tpe_mo_hvx.hip) and tpe_mo_exclusive4 (n_obj 4:
// tpe_mo_hvx4.hip) behind their n_obj checks: the same arguments, errors (under
// the entry's name `who`), upload, buffers and read-back.
int mo_exclusive_run(tpe_ctx* ctx, const char* who, const double* objectives, int64_t n, int32_t n_obj,
                     const double* reference, const double* constraints, int32_t n_con, int32_t mode, double* excl,
                     int32_t* n_overflow) {
    const std::string name(who);
    if (!objectives || !reference || !excl) return ctx->fail(TPE_ERR_ARG, name + ": null pointer");
    if (n < 1 || n > kMoMaxRows) return ctx->fail(TPE_ERR_ARG, name + ": n must be in [1, 2^20]");
    if (constraints && (n_con < 1 || n_con > kMoMaxCon))
        return ctx->fail(TPE_ERR_ARG, name + ": n_con must be in [1, 8]");
    if (mode != 0 && mode != 1) return ctx->fail(TPE_ERR_ARG, name + ": mode must be 0 or 1");
    Hvx4Ref ref4{};
    for (int m = 0; m < n_obj; ++m) {
        ref4.r[m] = reference[m];
        if (!(reference[m] - reference[m] == 0.0))
            return ctx->fail(TPE_ERR_ARG, name + ": the reference point must be finite");
    }
    const HvxRef ref{{ref4.r[0], ref4.r[1], ref4.r[2]}};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MoState* S = mo_of(ctx);
    const int32_t N = (int32_t)n;
    const size_t nf = (size_t)n * n_obj, ng = constraints ? (size_t)n * n_con : 0;
    HIPCHK(ctx, S->in.reserve(nf + ng));
    HIPCHK(ctx, S->in_h.resize(nf + ng));
    if (constraints) HIPCHK(ctx, S->v.reserve(n));
    HIPCHK(ctx, S->xflag.reserve(n));
    HIPCHK(ctx, S->xlive.reserve(n));
    HIPCHK(ctx, S->xhdr.reserve(kHvxHdr));
    HIPCHK(ctx, S->excl.reserve(n));
    HIPCHK(ctx, S->excl_h.resize(n));
    HIPCHK(ctx, S->xhdr_h.resize(kHvxHdr));
    double* d_F = S->in.p;

    // F (and G) in pinned memory: the call's one upload
    std::memcpy(S->in_h.data(), objectives, nf * sizeof(double));
    if (constraints) std::memcpy(S->in_h.data() + nf, constraints, ng * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(S->in.p, S->in_h.data(), (nf + ng) * sizeof(double), hipMemcpyHostToDevice, st));
    const unsigned row_blocks = blocks_of(n, kBlock);
    const unsigned slices = std::max(1u, std::min(row_blocks, (kMoBlocks + row_blocks - 1) / row_blocks));
    const int32_t per_slice = (int32_t)((n + slices - 1) / slices);
    const dim3 grid(row_blocks, blocks_of(n, per_slice));
    if (constraints) {
        // the rows that are dead or infeasible: NaN on the device copy
        hipLaunchKernelGGL(k_moc_prep, dim3(row_blocks), dim3(kBlock), 0, st, d_F, S->in.p + nf, N, n_obj, n_con,
                           S->v.p);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_obj == 4) {
        const int32_t cap = ctx->opt.mo_hvx_cap > 0 ? (int32_t)ctx->opt.mo_hvx_cap : kHvx4Cap;
        hvx4_launch(st, d_F, N, ref4, mode, cap, grid, per_slice, S->xflag.p, S->xlive.p, S->xhdr.p, S->excl.p);
    } else {
        const int32_t cap = ctx->opt.mo_hvx_cap > 0 ? (int32_t)ctx->opt.mo_hvx_cap : kHvxCap;
        hvx_launch(n_obj, st, d_F, N, ref, mode, cap, grid, per_slice, S->xflag.p, S->xlive.p, S->xhdr.p, S->excl.p);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(S->excl_h.data(), S->excl.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(S->xhdr_h.data(), S->xhdr.p, kHvxHdr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    std::memcpy(excl, S->excl_h.data(), (size_t)n * sizeof(double));
    if (n_overflow) *n_overflow = S->xhdr_h[1];
    return TPE_OK;
}

// tpe_mo_keys_hv (n_samples 0: the exact gains, tpe_mo_hv.hip) and
// tpe_mo_keys_hvs (n_samples > 0: the sampled ones, tpe_mo_hvs.hip) behind
// their n_obj and n_samples checks: the same arguments, errors (under the
// entry's name `who`), upload, dominance, sort and scatter pipeline and
// read-back.
int mo_keys_hv_run(tpe_ctx* ctx, const char* who, const double* objectives, int64_t n, int32_t n_obj,
                   const double* constraints, int32_t n_con, int32_t n_select, int32_t n_samples, double* keys,
                   int32_t* dominated_by, int32_t* dominates, double* violation, int32_t* picked, uint64_t* gains,
                   int32_t* n_picked) {
    const std::string name(who);
    const bool sampled = n_samples > 0;
    if (!objectives || !keys) return ctx->fail(TPE_ERR_ARG, name + ": null pointer");
    if (n < 1 || n > kMoMaxRows) return ctx->fail(TPE_ERR_ARG, name + ": n must be in [1, 2^20]");
    if (constraints && (n_con < 1 || n_con > kMoMaxCon))
        return ctx->fail(TPE_ERR_ARG, name + ": n_con must be in [1, 8]");
    if (n_select < 0 || n_select > kHvMaxPicks)
        return ctx->fail(TPE_ERR_ARG, name + ": n_select must be in [0, 64]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MoState* S = mo_of(ctx);
    const int32_t N = (int32_t)n;
    int32_t bits = 1;
    while (((int64_t)1 << bits) <= n) ++bits;
    // (n_select of 0 or past the rows: the keys are the old keys, nothing to select)
    const bool select = n_select > 0 && n_select < n;
    const size_t nf = (size_t)n * n_obj, ng = constraints ? (size_t)n * n_con : 0;
    HIPCHK(ctx, S->in.reserve(nf + ng));
    HIPCHK(ctx, S->in_h.resize(nf + ng));
    HIPCHK(ctx, S->keys.reserve(n));
    HIPCHK(ctx, S->cnt.reserve(2 * (size_t)n));
    HIPCHK(ctx, S->key.reserve(n));
    HIPCHK(ctx, S->key2.reserve(n));
    HIPCHK(ctx, S->keys_h.resize(n));
    HIPCHK(ctx, S->cnt_h.resize(2 * (size_t)n));
    if (constraints) {
        HIPCHK(ctx, S->v.reserve(n));
        HIPCHK(ctx, S->cntv.reserve(2 * (size_t)n));
        HIPCHK(ctx, S->v_h.resize(n));
    }
    HIPCHK(ctx, S->rank.reserve(nf));
    HIPCHK(ctx, S->lvl_r.reserve(nf));
    HIPCHK(ctx, S->lvl.reserve(2 * (size_t)n));
    HIPCHK(ctx, S->flag.reserve(n));
    HIPCHK(ctx, S->hdr.reserve(kHvHdr));
    HIPCHK(ctx, S->pick.reserve(kHvMaxPicks));
    HIPCHK(ctx, S->gain.reserve(kHvMaxPicks));
    HIPCHK(ctx, S->pick_h.resize(kHvHdr + kHvMaxPicks));
    HIPCHK(ctx, S->gain_h.resize(kHvMaxPicks));
    size_t sort_bytes = 0;
    hipcub::DoubleBuffer<uint64_t> kb(S->key.p, S->key2.p);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, kb, (int)N, 0, 3 * bits, st));
    HIPCHK(ctx, S->tmp.reserve(std::max<size_t>(sort_bytes, 1)));
    double* d_F = S->in.p;
    const double* d_G = S->in.p + nf;
    int32_t* d_by = S->cnt.p;
    int32_t* d_do = S->cnt.p + n;

    // F (and G) in pinned memory: the call's one upload
    std::memcpy(S->in_h.data(), objectives, nf * sizeof(double));
    if (constraints) std::memcpy(S->in_h.data() + nf, constraints, ng * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(S->in.p, S->in_h.data(), (nf + ng) * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(S->cnt.p, 0, 2 * (size_t)n * sizeof(int32_t), st));
    HIPCHK(ctx, hipMemsetAsync(S->rank.p, 0, nf * sizeof(uint32_t), st));
    const unsigned row_blocks = blocks_of(n, kBlock);
    const unsigned slices = std::max(1u, std::min(row_blocks, (kMoBlocks + row_blocks - 1) / row_blocks));
    const int32_t per_slice = (int32_t)((n + slices - 1) / slices);
    const dim3 grid(row_blocks, blocks_of(n, per_slice));
    if (constraints) {
        HIPCHK(ctx, hipMemsetAsync(S->cntv.p, 0, 2 * (size_t)n * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_moc_prep, dim3(row_blocks), dim3(kBlock), 0, st, d_F, d_G, N, n_obj, n_con, S->v.p);
        HIPCHK(ctx, hipGetLastError());
    } else {
        hv_launch_prep(st, d_F, N, n_obj);
        HIPCHK(ctx, hipGetLastError());
    }
    // counts and rank coordinates among the rank rows (every other row of the
    // device copy is NaN by now)
    if (sampled)
        hvs_launch_pairs(n_obj, grid, st, d_F, N, per_slice, d_by, d_do, S->rank.p);
    else
        hv_launch_pairs(n_obj, grid, st, d_F, N, per_slice, d_by, d_do, S->rank.p);
    HIPCHK(ctx, hipGetLastError());
    if (constraints) {
        launch_pairs<1>(grid, st, S->v.p, N, per_slice, S->cntv.p, S->cntv.p + n);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_moc_pack, dim3(row_blocks), dim3(kBlock), 0, st, S->v.p, N, bits, d_by, d_do,
                           S->cntv.p, S->key.p);
    } else {
        hipLaunchKernelGGL(k_mo_pack, dim3(row_blocks), dim3(kBlock), 0, st, d_F, N, n_obj, bits, d_by, d_do,
                           S->key.p);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(S->tmp.p, sort_bytes, kb, (int)N, 0, 3 * bits, st));
    if (constraints)
        hipLaunchKernelGGL(k_moc_scatter, dim3(row_blocks), dim3(kBlock), 0, st, kb.Current(), N, bits, S->keys.p,
                           d_by, d_do);
    else
        hipLaunchKernelGGL(k_mo_scatter, dim3(row_blocks), dim3(kBlock), 0, st, kb.Current(), N, bits, S->keys.p,
                           d_by, d_do);
    HIPCHK(ctx, hipGetLastError());
    if (select && sampled) {
        // the level at n_select on the device; its size sizes the coverage
        // matrix and its q the picks, so the header comes back first
        HvsBufs b{};
        b.sorted = kb.Current();
        b.v = constraints ? S->v.p : nullptr;
        b.rank = S->rank.p;
        b.hdr = S->hdr.p;
        b.lvl = S->lvl.p;
        b.lvl_r = S->lvl_r.p;
        b.flag = S->flag.p;
        b.pick = S->pick.p;
        b.gain = S->gain.p;
        b.keys = S->keys.p;
        hvs_launch_level(n_obj, st, b, N, bits, n_select);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(S->pick_h.data(), S->hdr.p, kHvHdr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));   // the first of the call's two synchronisations
        const int32_t a = S->pick_h[0], L = S->pick_h[1] - a, q = S->pick_h[2], n_f = S->pick_h[3];
        if (q > 0) {
            const size_t W = (size_t)n_samples / 64;
            if ((uint64_t)L * (uint64_t)n_samples > ((uint64_t)1 << 33))
                return ctx->fail(TPE_ERR_ARG, name + ": the coverage matrix of a level of L = " + std::to_string(L) +
                                                  " rows and n_samples = " + std::to_string(n_samples) +
                                                  " exceeds 1 GiB (L * n_samples > 2^33)");
            HIPCHK(ctx, S->hvs_bits.reserve(W * (size_t)L));
            HIPCHK(ctx, S->hvs_pts.reserve((size_t)n_obj * n_samples));
            HIPCHK(ctx, S->hvs_cov.reserve(W));
            HIPCHK(ctx, S->hvs_gain.reserve(L));
            HIPCHK(ctx, S->hvs_lo.reserve(kHvsMaxObj));
            HIPCHK(ctx, S->hvs_pick_t.reserve(kHvsMaxPicks));
            b.bits = S->hvs_bits.p;
            b.pts = S->hvs_pts.p;
            b.covered = S->hvs_cov.p;
            b.cgain = S->hvs_gain.p;
            b.lo = S->hvs_lo.p;
            b.pick_t = S->hvs_pick_t.p;
            HIPCHK(ctx, hipMemsetAsync(S->hvs_cov.p, 0, W * sizeof(uint64_t), st));
            HIPCHK(ctx, hipMemsetAsync(S->hvs_gain.p, 0, (size_t)L * sizeof(uint32_t), st));
            hvs_launch_select(n_obj, st, b, N, a, L, q, n_f, n_samples);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(S->pick_h.data() + kHvHdr, S->pick.p, q * sizeof(int32_t),
                                       hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipMemcpyAsync(S->gain_h.data(), S->gain.p, q * sizeof(unsigned long long),
                                       hipMemcpyDeviceToHost, st));
        }
    } else if (select) {
        // the level at n_select, its picks, and the keys of its rows -- all on the device
        hv_launch_select(n_obj, st, kb.Current(), N, bits, constraints ? S->v.p : nullptr, n_select, S->rank.p,
                         S->hdr.p, S->lvl.p, S->lvl_r.p, S->flag.p, S->keys.p, S->pick.p, S->gain.p);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(S->pick_h.data(), S->hdr.p, kHvHdr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(S->pick_h.data() + kHvHdr, S->pick.p, kHvMaxPicks * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(S->gain_h.data(), S->gain.p, kHvMaxPicks * sizeof(unsigned long long),
                                   hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(S->keys_h.data(), S->keys.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (dominated_by || dominates)
        HIPCHK(ctx, hipMemcpyAsync(S->cnt_h.data(), S->cnt.p, 2 * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   st));
    if (violation && constraints)
        HIPCHK(ctx, hipMemcpyAsync(S->v_h.data(), S->v.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation (sampled: its second)
    std::memcpy(keys, S->keys_h.data(), (size_t)n * sizeof(double));
    if (dominated_by) std::memcpy(dominated_by, S->cnt_h.data(), (size_t)n * sizeof(int32_t));
    if (dominates) std::memcpy(dominates, S->cnt_h.data() + n, (size_t)n * sizeof(int32_t));
    if (violation && constraints) std::memcpy(violation, S->v_h.data(), (size_t)n * sizeof(double));
    const int32_t q = select ? S->pick_h[2] : 0;
    for (int32_t k = 0; k < n_select; ++k) {
        if (picked) picked[k] = k < q ? S->pick_h[kHvHdr + k] : -1;
        if (gains) gains[k] = k < q ? (uint64_t)S->gain_h[k] : 0;
    }
    if (n_picked) *n_picked = q;
    return TPE_OK;
}

}  // namespace

extern "C" {

int tpe_mo_keys(tpe_ctx* ctx, const double* objectives, int64_t n, int32_t n_obj, double* keys,
                int32_t* dominated_by, int32_t* dominates) {
    if (!ctx) return TPE_ERR_ARG;
    if (!objectives || !keys) return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys: null pointer");
    if (n < 1 || n > kMoMaxRows) return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys: n must be in [1, 2^20]");
    if (n_obj < 1 || n_obj > kMoMaxObj) return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys: n_obj must be in [1, 8]");
    // (a multi-device context: its primary device)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MoState* S = mo_of(ctx);
    const int32_t N = (int32_t)n;
    int32_t bits = 1;
    while (((int64_t)1 << bits) <= n) ++bits;   // n itself fits: n - do of a row that dominates nobody, a NaN row's by
    const size_t nf = (size_t)n * n_obj;
    HIPCHK(ctx, S->F.reserve(nf));
    HIPCHK(ctx, S->keys.reserve(n));
    HIPCHK(ctx, S->cnt.reserve(2 * (size_t)n));
    HIPCHK(ctx, S->key.reserve(n));
    HIPCHK(ctx, S->key2.reserve(n));
    HIPCHK(ctx, S->keys_h.resize(n));
    HIPCHK(ctx, S->cnt_h.resize(2 * (size_t)n));
    size_t sort_bytes = 0;
    hipcub::DoubleBuffer<uint64_t> kb(S->key.p, S->key2.p);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, kb, (int)N, 0, 3 * bits, st));
    HIPCHK(ctx, S->tmp.reserve(std::max<size_t>(sort_bytes, 1)));
    int32_t* d_by = S->cnt.p;
    int32_t* d_do = S->cnt.p + n;

    HIPCHK(ctx, hipMemcpyAsync(S->F.p, objectives, nf * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(S->cnt.p, 0, 2 * (size_t)n * sizeof(int32_t), st));
    // row blocks x j-slices: enough workgroups for the chip, slices of whole
    // blocks of rows (10k rows: 40 x 26)
    const unsigned row_blocks = blocks_of(n, kBlock);
    const unsigned slices = std::max(1u, std::min(row_blocks, (kMoBlocks + row_blocks - 1) / row_blocks));
    const int32_t per_slice = (int32_t)((n + slices - 1) / slices);
    const dim3 grid(row_blocks, blocks_of(n, per_slice));
    launch_pairs_of(n_obj, grid, st, S->F.p, N, per_slice, d_by, d_do);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_mo_pack, dim3(row_blocks), dim3(kBlock), 0, st, S->F.p, N, n_obj, bits, d_by, d_do,
                       S->key.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(S->tmp.p, sort_bytes, kb, (int)N, 0, 3 * bits, st));
    hipLaunchKernelGGL(k_mo_scatter, dim3(row_blocks), dim3(kBlock), 0, st, kb.Current(), N, bits, S->keys.p, d_by,
                       d_do);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(S->keys_h.data(), S->keys.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (dominated_by || dominates)
        HIPCHK(ctx, hipMemcpyAsync(S->cnt_h.data(), S->cnt.p, 2 * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    std::memcpy(keys, S->keys_h.data(), (size_t)n * sizeof(double));
    if (dominated_by) std::memcpy(dominated_by, S->cnt_h.data(), (size_t)n * sizeof(int32_t));
    if (dominates) std::memcpy(dominates, S->cnt_h.data() + n, (size_t)n * sizeof(int32_t));
    return TPE_OK;
}

int tpe_mo_keys_constrained(tpe_ctx* ctx, const double* objectives, int64_t n, int32_t n_obj,
                            const double* constraints, int32_t n_con, double* keys, int32_t* dominated_by,
                            int32_t* dominates, double* violation) {
    if (!ctx) return TPE_ERR_ARG;
    if (!objectives || !constraints || !keys)
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys_constrained: null pointer");
    if (n < 1 || n > kMoMaxRows) return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys_constrained: n must be in [1, 2^20]");
    if (n_obj < 1 || n_obj > kMoMaxObj)
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys_constrained: n_obj must be in [1, 8]");
    if (n_con < 1 || n_con > kMoMaxCon)
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys_constrained: n_con must be in [1, 8]");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MoState* S = mo_of(ctx);
    const int32_t N = (int32_t)n;
    int32_t bits = 1;
    while (((int64_t)1 << bits) <= n) ++bits;
    const size_t nf = (size_t)n * n_obj, ng = (size_t)n * n_con;
    HIPCHK(ctx, S->in.reserve(nf + ng));
    HIPCHK(ctx, S->v.reserve(n));
    HIPCHK(ctx, S->cntv.reserve(2 * (size_t)n));
    HIPCHK(ctx, S->keys.reserve(n));
    HIPCHK(ctx, S->cnt.reserve(2 * (size_t)n));
    HIPCHK(ctx, S->key.reserve(n));
    HIPCHK(ctx, S->key2.reserve(n));
    HIPCHK(ctx, S->in_h.resize(nf + ng));
    HIPCHK(ctx, S->keys_h.resize(n));
    HIPCHK(ctx, S->cnt_h.resize(2 * (size_t)n));
    HIPCHK(ctx, S->v_h.resize(n));
    size_t sort_bytes = 0;
    hipcub::DoubleBuffer<uint64_t> kb(S->key.p, S->key2.p);
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, kb, (int)N, 0, 3 * bits, st));
    HIPCHK(ctx, S->tmp.reserve(std::max<size_t>(sort_bytes, 1)));
    double* d_F = S->in.p;
    const double* d_G = S->in.p + nf;
    int32_t* d_by = S->cnt.p;
    int32_t* d_do = S->cnt.p + n;
    int32_t* d_byv = S->cntv.p;
    int32_t* d_dov = S->cntv.p + n;

    // F and G side by side in pinned memory: the call's one upload
    std::memcpy(S->in_h.data(), objectives, nf * sizeof(double));
    std::memcpy(S->in_h.data() + nf, constraints, ng * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(S->in.p, S->in_h.data(), (nf + ng) * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(S->cnt.p, 0, 2 * (size_t)n * sizeof(int32_t), st));
    HIPCHK(ctx, hipMemsetAsync(S->cntv.p, 0, 2 * (size_t)n * sizeof(int32_t), st));
    const unsigned row_blocks = blocks_of(n, kBlock);
    const unsigned slices = std::max(1u, std::min(row_blocks, (kMoBlocks + row_blocks - 1) / row_blocks));
    const int32_t per_slice = (int32_t)((n + slices - 1) / slices);
    const dim3 grid(row_blocks, blocks_of(n, per_slice));
    hipLaunchKernelGGL(k_moc_prep, dim3(row_blocks), dim3(kBlock), 0, st, d_F, d_G, N, n_obj, n_con, S->v.p);
    HIPCHK(ctx, hipGetLastError());
    // the dominance counts among feasible rows (every other row is NaN by
    // now), then the rows of strictly smaller violation (a dead row's v is NaN)
    launch_pairs_of(n_obj, grid, st, d_F, N, per_slice, d_by, d_do);
    HIPCHK(ctx, hipGetLastError());
    launch_pairs<1>(grid, st, S->v.p, N, per_slice, d_byv, d_dov);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_moc_pack, dim3(row_blocks), dim3(kBlock), 0, st, S->v.p, N, bits, d_by, d_do, d_byv,
                       S->key.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortKeys(S->tmp.p, sort_bytes, kb, (int)N, 0, 3 * bits, st));
    hipLaunchKernelGGL(k_moc_scatter, dim3(row_blocks), dim3(kBlock), 0, st, kb.Current(), N, bits, S->keys.p, d_by,
                       d_do);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(S->keys_h.data(), S->keys.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (dominated_by || dominates)
        HIPCHK(ctx, hipMemcpyAsync(S->cnt_h.data(), S->cnt.p, 2 * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   st));
    if (violation)
        HIPCHK(ctx, hipMemcpyAsync(S->v_h.data(), S->v.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    std::memcpy(keys, S->keys_h.data(), (size_t)n * sizeof(double));
    if (dominated_by) std::memcpy(dominated_by, S->cnt_h.data(), (size_t)n * sizeof(int32_t));
    if (dominates) std::memcpy(dominates, S->cnt_h.data() + n, (size_t)n * sizeof(int32_t));
    if (violation) std::memcpy(violation, S->v_h.data(), (size_t)n * sizeof(double));
    return TPE_OK;
}

int tpe_mo_keys_hv(tpe_ctx* ctx, const double* objectives, int64_t n, int32_t n_obj, const double* constraints,
                   int32_t n_con, int32_t n_select, double* keys, int32_t* dominated_by, int32_t* dominates,
                   double* violation, int32_t* picked, uint64_t* gains, int32_t* n_picked) {
    if (!ctx) return TPE_ERR_ARG;
    if (n_obj != 2 && n_obj != 3) return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys_hv: n_obj must be 2 or 3");
    return mo_keys_hv_run(ctx, "tpe_mo_keys_hv", objectives, n, n_obj, constraints, n_con, n_select, 0, keys,
                          dominated_by, dominates, violation, picked, gains, n_picked);
}

int tpe_mo_keys_hvs(tpe_ctx* ctx, const double* objectives, int64_t n, int32_t n_obj, const double* constraints,
                    int32_t n_con, int32_t n_select, int32_t n_samples, double* keys, int32_t* dominated_by,
                    int32_t* dominates, double* violation, int32_t* picked, uint64_t* gains, int32_t* n_picked) {
    if (!ctx) return TPE_ERR_ARG;
    if (n_obj < 2 || n_obj > kHvsMaxObj) return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys_hvs: n_obj must be in [2, 8]");
    if (n_samples < 64 || n_samples > (1 << 20) || n_samples % 64)
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_keys_hvs: n_samples must be a multiple of 64 in [64, 2^20]");
    return mo_keys_hv_run(ctx, "tpe_mo_keys_hvs", objectives, n, n_obj, constraints, n_con, n_select, n_samples, keys,
                          dominated_by, dominates, violation, picked, gains, n_picked);
}

int tpe_mo_exclusive(tpe_ctx* ctx, const double* objectives, int64_t n, int32_t n_obj, const double* reference,
                     const double* constraints, int32_t n_con, int32_t mode, double* excl, int32_t* n_overflow) {
    if (!ctx) return TPE_ERR_ARG;
    if (n_obj != 2 && n_obj != 3) return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive: n_obj must be 2 or 3");
    return mo_exclusive_run(ctx, "tpe_mo_exclusive", objectives, n, n_obj, reference, constraints, n_con, mode, excl,
                            n_overflow);
}

int tpe_mo_exclusive4(tpe_ctx* ctx, const double* objectives, int64_t n, int32_t n_obj, const double* reference,
                      const double* constraints, int32_t n_con, int32_t mode, double* excl, int32_t* n_overflow) {
    if (!ctx) return TPE_ERR_ARG;
    if (n_obj != 4) return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive4: n_obj must be 4");
    return mo_exclusive_run(ctx, "tpe_mo_exclusive4", objectives, n, n_obj, reference, constraints, n_con, mode, excl,
                            n_overflow);
}

int tpe_mo_exclusive_mc(tpe_ctx* ctx, const double* objectives, int64_t n, int32_t n_obj, const double* reference,
                        const double* constraints, int32_t n_con, int32_t mode, int32_t n_samples, uint64_t* count,
                        uint64_t* covered, int32_t* n_alive) {
    if (!ctx) return TPE_ERR_ARG;
    if (!objectives || !reference || !count || !covered)
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive_mc: null pointer");
    if (n < 1 || n > kMoMaxRows) return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive_mc: n must be in [1, 2^20]");
    if (n_obj < 2 || n_obj > kHvmMaxObj)
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive_mc: n_obj must be in [2, 8]");
    if (constraints && (n_con < 1 || n_con > kMoMaxCon))
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive_mc: n_con must be in [1, 8]");
    if (mode != 0 && mode != 1) return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive_mc: mode must be 0 or 1");
    if (n_samples < 64 || n_samples > (1 << 20) || n_samples % 64)
        return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive_mc: n_samples must be a multiple of 64 in [64, 2^20]");
    HvmRef ref{};
    for (int m = 0; m < n_obj; ++m) {
        ref.r[m] = reference[m];
        if (!(reference[m] - reference[m] == 0.0))
            return ctx->fail(TPE_ERR_ARG, "tpe_mo_exclusive_mc: the reference point must be finite");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    MoState* S = mo_of(ctx);
    const int32_t N = (int32_t)n;
    const size_t nf = (size_t)n * n_obj, ng = constraints ? (size_t)n * n_con : 0;
    HIPCHK(ctx, S->in.reserve(nf + ng));
    HIPCHK(ctx, S->in_h.resize(nf + ng));
    if (constraints) HIPCHK(ctx, S->v.reserve(n));
    HIPCHK(ctx, S->hvm_T.reserve(((size_t)n + kHvmStep) * kHvmRow));
    HIPCHK(ctx, S->hvm_alive.reserve((size_t)n + kHvmStep));
    HIPCHK(ctx, S->hvm_lo.reserve(kHvmMaxObj));
    HIPCHK(ctx, S->hvm_samp.reserve((size_t)n_samples));
    HIPCHK(ctx, S->hvm_count.reserve((size_t)n + kHvmTail));
    HIPCHK(ctx, S->hvm_count_h.resize((size_t)n + kHvmTail));

    // F (and G) in pinned memory: the call's one upload
    std::memcpy(S->in_h.data(), objectives, nf * sizeof(double));
    if (constraints) std::memcpy(S->in_h.data() + nf, constraints, ng * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(S->in.p, S->in_h.data(), (nf + ng) * sizeof(double), hipMemcpyHostToDevice, st));
    if (constraints) {
        // the rows that are dead or infeasible: NaN on the device copy
        hipLaunchKernelGGL(k_moc_prep, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, st, S->in.p, S->in.p + nf, N,
                           n_obj, n_con, S->v.p);
        HIPCHK(ctx, hipGetLastError());
    }
    const HvmBufs b{S->in.p, S->hvm_lo.p, S->hvm_T.p, S->hvm_alive.p, S->hvm_samp.p, S->hvm_count.p};
    HIPCHK(ctx, hvm_launch(n_obj, st, b, N, ref, mode, n_samples));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(S->hvm_count_h.data(), S->hvm_count.p, ((size_t)n + kHvmTail) * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the call's one synchronisation
    for (int64_t i = 0; i < n; ++i) count[i] = (uint64_t)S->hvm_count_h[(size_t)i];
    *covered = (uint64_t)S->hvm_count_h[(size_t)n];
    if (n_alive) *n_alive = (int32_t)S->hvm_count_h[(size_t)n + 1];
    return TPE_OK;
}

}  // extern "C"
