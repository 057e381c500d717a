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
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"

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

}  // extern "C"
