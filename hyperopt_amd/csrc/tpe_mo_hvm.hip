// tpe_mo_hvm.hip -- the sampled hypervolume indicator, two to eight objectives
// (include/hyperopt_tpe.h, tpe_mo_exclusive_mc; tpe.hypervolume(method=
// 'sampled')): raw rows against a reference point, counted on a fixed set of
// Philox sample points on a lattice of 2^32 steps per axis.
//
// Row i is valid as in tpe_mo_exclusive.  lo[m] = the valid rows' minimum on
// axis m, span[m] = reference[m] - lo[m], T[i][m] = ceil(((F[i][m] - lo[m]) /
// span[m]) * 2^32) -- fp64, each operation rounded on its own -- an integer in
// [0, 2^32]; a valid row with a T of 2^32 is thin, every other valid row alive.
// Sample s has x[s][m] = word m % 4 of philox4x32_10 with counter (s, m / 4, 0,
// TPE_MO_HVM_STREAM) under the key (TPE_MO_HVS_KEY0, TPE_MO_HVS_KEY1); an alive
// row covers s iff x[s][m] >= T[i][m] on every axis.  Integers from T on.
//
// Kernels
//   k_hvm_prep       a thread per row: valid -> alive[i]; count[i] = 0, the two
//                    words behind count zeroed
//   k_hvm_lo         a workgroup per axis: the minimum over the valid rows (wave
//                    shuffles, then one LDS slot a wave; a min is order-free)
//   k_hvm_thresh     a thread per row: T[i][0 .. 8) as uint32, row-major, the
//                    words past M zero; the byte alive[i] cleared for a thin row; the
//                    alive rows counted, one atomicAdd a wave
//   k_hvm_cover<M, MODE>  grid (blocks of 4 waves of samples, row slices): lane l
//                    of a wave holds one sample in M VGPRs, drawn in the kernel
//                    (one Philox call per four axes; nothing is read from
//                    memory for it).  The row index is uniform over the wave:
//                    four rows' alive bytes (one word; a slice starts at a
//                    multiple of 4) and a row's words come by scalar loads, a dead
//                    row is a scalar branch, a row costs M unsigned compares
//                    whose 64-bit results the scalar unit ANDs and keeps as
//                    lane masks: covered once, covered twice.  Only a row that
//                    is some lane's first covering row costs more vector work
//                    (rows ascend, so those get rare fast).  Mode 0 leaves the
//                    loop when every lane has a row, mode 1 when every lane
//                    has two.  The exit is looked at every kHvmStep rows.  A
//                    slice merges by one integer atomic per lane:
//                    atomicMin(first[s]) or one 64-bit atomicAdd of (covers
//                    clamped to 2) << 32 | (the row when it is the only one) --
//                    the sum over slices has 1 on top exactly when one row of
//                    all covers s, and then that row below.  Order-free.
//   k_hvm_count<MODE>     a thread per sample: its row (none: not counted);
//                    lanes that hold the same row are found by ballot and one of
//                    them adds their number to count[row] -- early rows own
//                    most samples, so a wave sends a few atomics, not 64; the
//                    covered samples by one atomicAdd a wave
// No LDS past k_hvm_lo's four slots, no matrix instruction (the predicate is
// M integer compares), no cooperative launch, no workgroup waits on another.
#include <hip/hip_runtime.h>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"
#include "tpe_device.h"
#include "tpe_mo_hvm.h"

namespace tpe_rt {

namespace {

typedef unsigned long long u64;

constexpr uint32_t kNone = 0xFFFFFFFFu;     // no row: past every row index (n <= 2^20)

__global__ __launch_bounds__(kBlock) void k_hvm_prep(const double* __restrict__ F, int32_t n, int32_t n_obj,
                                                     HvmRef ref, unsigned char* __restrict__ alive,
                                                     uint32_t* __restrict__ count) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i == 0)
        for (int q = 0; q < kHvmTail; ++q) count[n + q] = 0;
    if (i >= n) return;
    bool ok = true;
    for (int m = 0; m < n_obj; ++m) {
        const double f = F[(size_t)i * n_obj + m];
        ok &= f > -__builtin_inf() && f < ref.r[m];   // (a NaN fails both)
    }
    alive[i] = ok ? 1 : 0;
    count[i] = 0;
}

// lo[m], m = blockIdx.x; +inf when no row is valid (k_hvm_thresh then has no row to work on)
__global__ __launch_bounds__(kBlock) void k_hvm_lo(const double* __restrict__ F, int32_t n, int32_t n_obj,
                                                   const unsigned char* __restrict__ alive,
                                                   double* __restrict__ lo) {
    __shared__ double slot[kBlock / 64];
    const int m = (int)blockIdx.x;
    double best = __builtin_inf();
    for (int32_t i = (int32_t)threadIdx.x; i < n; i += kBlock)
        if (alive[i]) best = fmin(best, F[(size_t)i * n_obj + m]);
#pragma unroll
    for (int o = 32; o; o >>= 1) best = fmin(best, __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) best = fmin(best, slot[w]);
        lo[m] = best;
    }
}

__global__ __launch_bounds__(kBlock) void k_hvm_thresh(const double* __restrict__ F, int32_t n, int32_t n_obj,
                                                       HvmRef ref, const double* __restrict__ lo,
                                                       uint32_t* __restrict__ T,
                                                       unsigned char* __restrict__ alive,
                                                       uint32_t* __restrict__ count) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    bool live = i < n && alive[i] != 0;
    if (i < n) {
        uint32_t t[kHvmRow];
#pragma unroll
        for (int m = 0; m < kHvmRow; ++m) t[m] = 0;
        if (live) {
#pragma unroll
            for (int m = 0; m < kHvmRow; ++m) {
                if (m < n_obj) {
                    const double l = lo[m];
                    const double span = ref.r[m] - l;
                    const double d = F[(size_t)i * n_obj + m] - l;
                    const double q = d / span;
                    const double c = ceil(q * 4294967296.0);      // in [0, 2^32]
                    live &= c < 4294967296.0;
                    t[m] = c < 4294967296.0 ? (uint32_t)c : kNone;
                }
            }
            if (!live) alive[i] = 0;                              // thin
        }
        uint4* row = reinterpret_cast<uint4*>(T + (size_t)i * kHvmRow);
        row[0] = make_uint4(t[0], t[1], t[2], t[3]);
        row[1] = make_uint4(t[4], t[5], t[6], t[7]);
    }
    const u64 b = __ballot(live);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count + n + 1, (uint32_t)__popcll(b));
}

template <int M, int MODE>
__global__ __launch_bounds__(kBlock) void k_hvm_cover(const uint32_t* __restrict__ T,
                                                      const uint32_t* __restrict__ alive4, int32_t n,
                                                      int32_t per_slice, int32_t S, uint32_t* __restrict__ first,
                                                      u64* __restrict__ tag) {
    const int32_t s = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (s >= S) return;                              // (S is a multiple of 64: uniform over the wave; no barrier)
    uint32_t x[M];
    {
        const tpe::U4 w = tpe::philox4x32_10(tpe::U4{(uint32_t)s, 0u, 0u, (uint32_t)TPE_MO_HVM_STREAM},
                                             (uint32_t)TPE_MO_HVS_KEY0, (uint32_t)TPE_MO_HVS_KEY1);
        const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int m = 0; m < (M < 4 ? M : 4); ++m) x[m] = word[m];
    }
    if (M > 4) {
        const tpe::U4 w = tpe::philox4x32_10(tpe::U4{(uint32_t)s, 1u, 0u, (uint32_t)TPE_MO_HVM_STREAM},
                                             (uint32_t)TPE_MO_HVS_KEY0, (uint32_t)TPE_MO_HVS_KEY1);
        const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int m = 4; m < M; ++m) x[m] = word[m - 4];
    }
    const int32_t j0 = (int32_t)blockIdx.y * per_slice;          // (uniform over the workgroup)
    const int32_t j1 = min(n, j0 + per_slice);
    // The lanes' predicates live in scalar registers, a bit a lane: a compare
    // writes its 64 results there, the axes are ANDed and the states kept by
    // the scalar unit.  `once`: the lanes with a covering row so far, `twice`
    // (mode 1): those with two.  Only a row that is some lane's first costs
    // vector work past its M compares: `row` takes i in those lanes.
    const u64 full = __ballot(true), bit = (u64)1 << (threadIdx.x & 63);
    u64 once = 0, twice = 0;
    uint32_t row = kNone;
    for (int32_t i0 = j0; i0 < j1; i0 += kHvmStep) {
        const uint32_t a4 = alive4[i0 / kHvmStep];   // (the bytes of rows i0 .. i0 + 3; j0 is a multiple of 4)
#pragma unroll
        for (int k = 0; k < kHvmStep; ++k) {
            const int32_t i = i0 + k;
            if (i < j1 && ((a4 >> (8 * k)) & 0xFFu)) {
                const uint32_t* __restrict__ t = T + (size_t)i * kHvmRow;
                u64 cov = __ballot(x[0] >= t[0]);
#pragma unroll
                for (int m = 1; m < M; ++m) cov &= __ballot(x[m] >= t[m]);
                const u64 fresh = cov & ~once;
                if (MODE == 1) twice |= cov & once;
                once |= cov;
                if (fresh) row = (fresh & bit) ? (uint32_t)i : row;
            }
        }
        if ((MODE == 0 ? once : twice) == full) break;
    }
    if (MODE == 0) {
        if (row != kNone) atomicMin(first + s, row);
    } else {
        if (row != kNone) atomicAdd(tag + s, (twice & bit) ? (u64)2 << 32 : ((u64)1 << 32) | (u64)row);
    }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_hvm_count(const uint32_t* __restrict__ first,
                                                      const u64* __restrict__ tag, int32_t S, int32_t n,
                                                      uint32_t* __restrict__ count) {
    const int32_t s = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const int lane = (int)(threadIdx.x & 63);
    uint32_t row = kNone;
    bool cov = false;
    if (s < S) {
        if (MODE == 0) {
            row = first[s];
            cov = row != kNone;
        } else {
            const u64 t = tag[s];
            cov = (t >> 32) != 0;
            row = (t >> 32) == 1 ? (uint32_t)t : kNone;
        }
    }
    const u64 c = __ballot(cov);
    if (lane == 0 && c) atomicAdd(count + n, (uint32_t)__popcll(c));
    bool live = row < (uint32_t)n;
    u64 left;
    while ((left = __ballot(live)) != 0) {           // (uniform: the wave stays whole)
        const int leader = __ffsll(left) - 1;
        const uint32_t r = (uint32_t)__shfl((int)row, leader);
        const u64 same = __ballot(live && row == r);
        if (lane == leader) atomicAdd(count + r, (uint32_t)__popcll(same));
        live = live && row != r;
    }
}

template <int M>
void launch_cover(dim3 grid, hipStream_t st, const HvmBufs& b, int32_t n, int32_t per_slice, int32_t mode,
                  int32_t S) {
    uint32_t* first = reinterpret_cast<uint32_t*>(b.samp);
    u64* tag = reinterpret_cast<u64*>(b.samp);
    const uint32_t* alive4 = reinterpret_cast<const uint32_t*>(b.alive);
    if (mode == 0)
        hipLaunchKernelGGL((k_hvm_cover<M, 0>), grid, dim3(kBlock), 0, st, b.T, alive4, n, per_slice, S, first, tag);
    else
        hipLaunchKernelGGL((k_hvm_cover<M, 1>), grid, dim3(kBlock), 0, st, b.T, alive4, n, per_slice, S, first, tag);
}

}  // namespace

hipError_t hvm_launch(int32_t n_obj, hipStream_t st, const HvmBufs& b, int32_t n, HvmRef ref, int32_t mode,
                      int32_t S) {
    const dim3 rows((unsigned)((n + kBlock - 1) / kBlock)), samples((unsigned)((S + kBlock - 1) / kBlock));
    // first[s] = no row (every byte 0xFF), or the tags zero
    const hipError_t e = mode == 0 ? hipMemsetAsync(b.samp, 0xFF, (size_t)S * sizeof(uint32_t), st)
                                   : hipMemsetAsync(b.samp, 0, (size_t)S * sizeof(uint64_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hvm_prep, rows, dim3(kBlock), 0, st, b.F, n, n_obj, ref, b.alive, b.count);
    hipLaunchKernelGGL(k_hvm_lo, dim3((unsigned)n_obj), dim3(kBlock), 0, st, b.F, n, n_obj, b.alive, b.lo);
    hipLaunchKernelGGL(k_hvm_thresh, rows, dim3(kBlock), 0, st, b.F, n, n_obj, ref, b.lo, b.T, b.alive, b.count);
    const int32_t slices = hvm_slices(n, S);
    const int32_t per_slice = ((n + slices - 1) / slices + kHvmStep - 1) / kHvmStep * kHvmStep;
    const dim3 grid(samples.x, (unsigned)((n + per_slice - 1) / per_slice));
    switch (n_obj) {
        case 2: launch_cover<2>(grid, st, b, n, per_slice, mode, S); break;
        case 3: launch_cover<3>(grid, st, b, n, per_slice, mode, S); break;
        case 4: launch_cover<4>(grid, st, b, n, per_slice, mode, S); break;
        case 5: launch_cover<5>(grid, st, b, n, per_slice, mode, S); break;
        case 6: launch_cover<6>(grid, st, b, n, per_slice, mode, S); break;
        case 7: launch_cover<7>(grid, st, b, n, per_slice, mode, S); break;
        default: launch_cover<8>(grid, st, b, n, per_slice, mode, S); break;
    }
    const uint32_t* first = reinterpret_cast<const uint32_t*>(b.samp);
    const u64* tag = reinterpret_cast<const u64*>(b.samp);
    if (mode == 0)
        hipLaunchKernelGGL(k_hvm_count<0>, samples, dim3(kBlock), 0, st, first, tag, S, n, b.count);
    else
        hipLaunchKernelGGL(k_hvm_count<1>, samples, dim3(kBlock), 0, st, first, tag, S, n, b.count);
    return hipSuccess;
}

}  // namespace tpe_rt
