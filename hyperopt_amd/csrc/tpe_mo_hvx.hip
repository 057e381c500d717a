// tpe_mo_hvx.hip -- the hypervolume indicator's exclusive volumes
// (include/hyperopt_tpe.h, tpe_mo_exclusive; tpe.hypervolume): for every valid
// row i of F [n][M], M 2 or 3, all minimised, against the reference point r,
//     excl(i | J) = vol(box i) - vol(union over j in J of box j cut by box i),
// box i = prod_m [F[i][m], r[m]), J the valid rows before i (mode 0) or every
// other valid row (mode 1).  fp64 throughout, compiled without contraction:
// every difference, product and sum below is rounded on its own, in the order
// written, so the same input gives the same bits on every run and the numpy
// builder (posterior.mo_exclusive) gives them too.
//
// The rule, for a row i that no row of J weakly dominates (a = F[i]):
//   clip   c_j = max(F[j], a) per axis, j in J;
//   keep   the distinct minimal elements of {c_j} (no other c weakly below);
//   M = 2  scan the kept points by ascending x with cx = a_x, cy = r_y, A = 0:
//          a point with y < cy adds (x - cx) (cy - a_y) to A and becomes
//          (cx, cy); at the end A += (r_x - cx) (cy - a_y).  excl = A: the part
//          of box i under the staircase, summed left to right;
//   M = 3  the kept points by ascending z: z_0 <= .. <= z_{k-1}.  Slab s = 0 .. k
//          spans [z_{s-1}, z_s) (z_{-1} = a_z, z_k = r_z); its area A_s is the
//          M = 2 scan over the kept points of z-rank < s.  excl = sum over s,
//          ascending, of (z_s - z_{s-1}) A_s.
// All terms are >= 0: no subtraction of two volumes anywhere.
//
// Kernels (one stream, no cooperative launch, no workgroup waits on another)
//   k_hvx_prep<M>   a thread per row: a row with a non-finite value or one not
//                   below r is set to NaN on the device copy (IEEE comparisons
//                   then drop it everywhere); flag 2 for it, 0 otherwise;
//                   excl = 0; the header zeroed
//   k_hvx_dom<M>    all pairs, split as k_mo_pairs splits them (row blocks x
//                   j-slices, row i in registers, rows j by wave-uniform loads):
//                   flag[i] = 1 when a row of J is weakly below row i.  Mode 0
//                   stops a slice at the block's last row
//   k_hvx_compact   the rows with flag 0 -- the live rows: the front of their
//                   prefix (mode 0) or the front without duplicates (mode 1) --
//                   into a list, one atomicAdd per wave (the list's order does
//                   not reach any result)
//   k_hvx_excl<M>   a fixed grid of workgroups, each taking live rows l, l +
//                   grid, ..: streams J in chunks of 256 rows (a thread a row),
//                   clips, drops what the kept set weakly dominates, appends the
//                   survivors (ballot prefix), prunes the set against the new
//                   points and compacts it; then bitonic sorts of 16-bit indices
//                   by z and by (x, y), a lane per slab for the areas, and one
//                   lane summing the slabs in ascending order.
// LDS of k_hvx_excl<3>, per workgroup: points (1024 + 256) x 24 B = 30 720,
// slab terms 1025 x 8 = 8 200, three index arrays 3 x 2 048, alive bytes 1 280,
// counters 1 056: 47.4 KB -- three workgroups on a CU's 160 KB, 12 waves of its
// 32 (the kernel is bound by the stream of rows and LDS broadcasts, not by
// occupancy).  M = 2: 24.9 KB (16 B points, no z arrays, one term).  A live row whose kept set exceeds the capacity
// after a prune gets NaN and counts in hdr[1]; the caller recomputes it.
#include <hip/hip_runtime.h>

#include "tpe_ctx.h"
#include "tpe_mo_hvx.h"

namespace tpe_rt {

namespace {

constexpr int kHvxBuf = kHvxCap + kBlock;         // the kept set plus one chunk's survivors
constexpr int kHvxPer = kHvxBuf / kBlock;         // entries a thread moves in a compaction
constexpr int kHvxWaves = kBlock / 64;
constexpr unsigned kHvxPad = 0xFFFFu;             // index of a padding slot of a sort: past every point
constexpr unsigned kHvxGrid = 768;                // workgroups of k_hvx_excl: 3 per CU
static_assert(kHvxBuf % kBlock == 0, "a thread moves whole entries");

template <int M>
__global__ __launch_bounds__(kBlock) void k_hvx_prep(double* __restrict__ F, int32_t n, HvxRef ref,
                                                     int32_t* __restrict__ flag, int32_t* __restrict__ hdr,
                                                     double* __restrict__ excl) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i == 0)
        for (int q = 0; q < kHvxHdr; ++q) hdr[q] = 0;
    if (i >= n) return;
    bool ok = true;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const double f = F[(size_t)i * M + m];
        ok &= f > -__builtin_inf() && f < ref.r[m];   // (a NaN fails both)
    }
    if (!ok)
#pragma unroll
        for (int m = 0; m < M; ++m) F[(size_t)i * M + m] = __builtin_nan("");
    flag[i] = ok ? 0 : 2;
    excl[i] = 0.0;
}

template <int M>
__global__ __launch_bounds__(kBlock) void k_hvx_dom(const double* __restrict__ F, int32_t n, int32_t per_slice,
                                                    int32_t mode, int32_t* __restrict__ flag) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    // a lane past the rows, and a row that is not valid, compares NaNs: never dominated
    double fi[M];
#pragma unroll
    for (int m = 0; m < M; ++m) fi[m] = i < n ? F[(size_t)i * M + m] : __builtin_nan("");
    const int32_t j0 = (int32_t)blockIdx.y * per_slice;          // (uniform over the workgroup)
    int32_t j1 = min(n, j0 + per_slice);
    if (mode == 0) j1 = min(j1, (int32_t)((blockIdx.x + 1) * kBlock));   // no row of the block has a later j
    bool dom = false;
#pragma unroll 4
    for (int32_t j = j0; j < j1; ++j) {
        const double* __restrict__ fj = F + (size_t)j * M;
        bool le = true;
#pragma unroll
        for (int m = 0; m < M; ++m) le &= fj[m] <= fi[m];
        dom |= le && (mode == 0 ? j < i : j != i);
    }
    if (dom && i < n) flag[i] = 1;   // (every writer writes 1)
}

__global__ __launch_bounds__(kBlock) void k_hvx_compact(const int32_t* __restrict__ flag, int32_t n,
                                                        int32_t* __restrict__ live, int32_t* __restrict__ hdr) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const bool is_live = i < n && flag[i] == 0;
    const unsigned long long bal = __ballot(is_live);
    const int lane = (int)(threadIdx.x & 63);
    int32_t base = 0;
    if (lane == 0 && bal) base = atomicAdd(hdr, (int32_t)__popcll(bal));
    base = __shfl(base, 0, 64);
    if (is_live) live[base + (int32_t)__popcll(bal & (((unsigned long long)1 << lane) - 1))] = i;
}

// ia before ib by axis A, then axis B (B < 0: none), then index; padding last
template <int M, int A, int B>
__device__ inline bool hvx_before(const double* pts, unsigned ia, unsigned ib) {
    if (ia == kHvxPad) return false;
    if (ib == kHvxPad) return true;
    const double ka = pts[ia * M + A], kb = pts[ib * M + A];
    if (ka != kb) return ka < kb;
    if (B >= 0) {
        const double la = pts[ia * M + (B >= 0 ? B : 0)], lb = pts[ib * M + (B >= 0 ? B : 0)];
        if (la != lb) return la < lb;
    }
    return ia < ib;
}

// ord[0 .. np), np a power of two <= kHvxCap: the indices k .. np - 1 are
// padding.  Ends with a barrier.
template <int M, int A, int B>
__device__ inline void hvx_sort(const double* pts, uint16_t* ord, int k, int np) {
    for (int e = (int)threadIdx.x; e < np; e += kBlock) ord[e] = (uint16_t)(e < k ? (unsigned)e : kHvxPad);
    __syncthreads();
    for (int size = 2; size <= np; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = (int)threadIdx.x; t < (np >> 1); t += kBlock) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;   // hi < np
                const bool up = (lo & size) == 0;
                const unsigned x = ord[lo], y = ord[hi];
                if (hvx_before<M, A, B>(pts, y, x) == up) {
                    ord[lo] = (uint16_t)y;
                    ord[hi] = (uint16_t)x;
                }
            }
            __syncthreads();
        }
}

template <int M>
__global__ __launch_bounds__(kBlock) void k_hvx_excl(const double* __restrict__ F, int32_t n, HvxRef ref,
                                                     int32_t mode, int32_t cap, const int32_t* __restrict__ live,
                                                     int32_t* __restrict__ hdr, double* __restrict__ excl) {
    __shared__ double pts[kHvxBuf * M];
    __shared__ double term[kHvxCap + 1];
    __shared__ uint16_t zord[kHvxCap], xord[kHvxCap], zrank[kHvxCap];
    __shared__ unsigned char alive[kHvxBuf];
    __shared__ int32_t cnt[kBlock];
    __shared__ int32_t wtot[2][kHvxWaves];
    const int T = (int)threadIdx.x, lane = T & 63, w = T >> 6;
    const int32_t n_live = min(hdr[0], n);
    for (int32_t l = (int32_t)blockIdx.x; l < n_live; l += (int32_t)gridDim.x) {
        const int32_t i = live[l];
        double a[M];
#pragma unroll
        for (int m = 0; m < M; ++m) a[m] = F[(size_t)i * M + m];
        const int32_t jend = mode == 0 ? i : n;
        int k = 0;                 // the kept set pts[0 .. k): the same value in every thread
        bool over = false;
        int par = 0;
        for (int32_t j0 = 0; j0 < jend; j0 += kBlock, par ^= 1) {
            const int32_t j = j0 + T;
            bool have = j < jend && j != i;
            double c[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double f = have ? F[(size_t)j * M + m] : __builtin_nan("");
                have = have && f < ref.r[m];          // (a row that is not valid is NaN)
                c[m] = f > a[m] ? f : a[m];
            }
            for (int e = 0; have && e < k; ++e) {     // weakly dominated by a kept point: gone
                bool le = true;
#pragma unroll
                for (int m = 0; m < M; ++m) le &= pts[e * M + m] <= c[m];
                have = !le;
            }
            const unsigned long long bal = __ballot(have);
            if (lane == 0) wtot[par][w] = (int32_t)__popcll(bal);
            __syncthreads();
            int ns = 0, base = 0;
#pragma unroll
            for (int q = 0; q < kHvxWaves; ++q) {
                const int v = wtot[par][q];
                base += q < w ? v : 0;
                ns += v;
            }
            if (ns == 0) continue;                    // (uniform; wtot[par] is rewritten two barriers on at the earliest)
            // the survivors behind the kept set: k + ns <= cap + 256 entries
            if (have) {
                const int pos = k + base + (int)__popcll(bal & (((unsigned long long)1 << lane) - 1));
#pragma unroll
                for (int m = 0; m < M; ++m) pts[pos * M + m] = c[m];
            }
            __syncthreads();
            const int tot = k + ns;
            // an entry dies when a new point lies weakly below it (equal points: the later one)
            for (int e = T; e < tot; e += kBlock) {
                double p[M];
#pragma unroll
                for (int m = 0; m < M; ++m) p[m] = pts[e * M + m];
                bool dead = false;
                for (int q = k; q < tot && !dead; ++q) {
                    bool le = true, lt = false;
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const double v = pts[q * M + m];
                        le &= v <= p[m];
                        lt |= v < p[m];
                    }
                    dead = q != e && le && (lt || q < e);
                }
                alive[e] = dead ? 0 : 1;
            }
            __syncthreads();
            // stable compaction: a thread holds kHvxPer consecutive entries in registers
            double reg[kHvxPer][M];
            bool ok[kHvxPer];
            int mine = 0;
#pragma unroll
            for (int u = 0; u < kHvxPer; ++u) {
                const int e = T * kHvxPer + u;        // < kHvxBuf
                ok[u] = e < tot && alive[e];
#pragma unroll
                for (int m = 0; m < M; ++m) reg[u][m] = ok[u] ? pts[e * M + m] : 0.0;
                mine += ok[u] ? 1 : 0;
            }
            cnt[T] = mine;
            __syncthreads();
            int off = 0, total = 0;
            for (int q = 0; q < kBlock; ++q) {
                const int v = cnt[q];
                off += q < T ? v : 0;
                total += v;
            }
#pragma unroll
            for (int u = 0; u < kHvxPer; ++u)
                if (ok[u]) {                          // off < total <= tot <= kHvxBuf
#pragma unroll
                    for (int m = 0; m < M; ++m) pts[off * M + m] = reg[u][m];
                    ++off;
                }
            __syncthreads();
            k = total;
            if (k > cap) {                            // (uniform)
                over = true;
                break;
            }
        }
        if (over) {
            if (T == 0) {
                excl[i] = __builtin_nan("");
                atomicAdd(hdr + 1, 1);
            }
            __syncthreads();
            continue;
        }
        __syncthreads();
        // k <= cap <= kHvxCap
        int np = 1;
        while (np < k) np <<= 1;
        if (M == 3) {
            hvx_sort<M, M - 1, -1>(pts, zord, k, np);
            for (int p = T; p < k; p += kBlock) zrank[zord[p]] = (uint16_t)p;
        }
        hvx_sort<M, 0, 1>(pts, xord, k, np);
        // a lane per slab (M = 2: one slab, every kept point in it)
        const int nslab = M == 3 ? k + 1 : 1;
        for (int s = T; s < nslab; s += kBlock) {
            double cx = a[0], cy = ref.r[1], area = 0.0;
            for (int p = 0; p < k; ++p) {
                const unsigned e = xord[p];
                if (M == 3 && (int)zrank[e] >= s) continue;
                const double y = pts[e * M + 1];
                if (y < cy) {
                    const double x = pts[e * M];
                    area = area + (x - cx) * (cy - a[1]);
                    cx = x;
                    cy = y;
                }
            }
            area = area + (ref.r[0] - cx) * (cy - a[1]);
            if (M == 3) {
                const double lo = s == 0 ? a[M - 1] : pts[zord[s - 1] * M + M - 1];
                const double hi = s == k ? ref.r[M - 1] : pts[zord[s] * M + M - 1];
                term[s] = (hi - lo) * area;
            } else {
                term[s] = area;
            }
        }
        __syncthreads();
        if (T == 0) {
            double v = term[0];
            for (int s = 1; s < nslab; ++s) v = v + term[s];
            excl[i] = v;
        }
        __syncthreads();
    }
}

template <int M>
void hvx_launch_m(hipStream_t st, double* F, int32_t n, HvxRef ref, int32_t mode, int32_t cap, dim3 pair_grid,
                  int32_t per_slice, int32_t* flag, int32_t* live, int32_t* hdr, double* excl) {
    const dim3 rows((unsigned)((n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_hvx_prep<M>, rows, dim3(kBlock), 0, st, F, n, ref, flag, hdr, excl);
    hipLaunchKernelGGL(k_hvx_dom<M>, pair_grid, dim3(kBlock), 0, st, F, n, per_slice, mode, flag);
    hipLaunchKernelGGL(k_hvx_compact, rows, dim3(kBlock), 0, st, flag, n, live, hdr);
    hipLaunchKernelGGL(k_hvx_excl<M>, dim3(std::min<unsigned>(kHvxGrid, (unsigned)n)), dim3(kBlock), 0, st, F, n,
                       ref, mode, cap, live, hdr, excl);
}

}  // namespace

void hvx_launch(int32_t n_obj, hipStream_t st, double* F, int32_t n, HvxRef ref, int32_t mode, int32_t cap,
                dim3 pair_grid, int32_t per_slice, int32_t* flag, int32_t* live, int32_t* hdr, double* excl) {
    cap = std::max(1, std::min(cap, kHvxCap));
    if (n_obj == 2)
        hvx_launch_m<2>(st, F, n, ref, mode, cap, pair_grid, per_slice, flag, live, hdr, excl);
    else
        hvx_launch_m<3>(st, F, n, ref, mode, cap, pair_grid, per_slice, flag, live, hdr, excl);
}

}  // namespace tpe_rt
