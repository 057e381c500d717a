// tpe_mo_hvx4.hip -- the hypervolume indicator's exclusive volumes with four
// objectives (include/hyperopt_tpe.h, tpe_mo_exclusive4; tpe.hypervolume): for
// every valid row i of F [n][4], all minimised, against the reference point r,
//     excl(i | J) = vol(box i) - vol(union over j in J of box j cut by box i),
// box i = prod_m [F[i][m], r[m]), J the valid rows before i (mode 0) or every
// other valid row (mode 1).  fp64 throughout, compiled without contraction:
// every difference, product and sum below is rounded on its own, in the order
// written, so the same input gives the same bits on every run and the numpy
// builder (posterior.mo_exclusive) gives them too.
//
// The rule, for a row i that no row of J weakly dominates (a = F[i]; the axes
// are x, y, z, w):
//   clip   c_j = max(F[j], a) per axis, j in J;
//   keep   the distinct minimal elements of {c_j}: k points;
//   rank   w-rank: the position by ascending w, w_0 <= .. <= w_{k-1}; z-rank:
//          the position by ascending z, z_0 <= .. <= z_{k-1}; the x order: by
//          (x, y).  (Equal keys may stand in any order: they bound a slab of
//          thickness 0, whose term is 0.)
//   cell   (t, s), t, s = 0 .. k: A[t][s] = the two-objective scan -- cx = a_x,
//          cy = r_y, area = 0; a point with y < cy adds (x - cx) (cy - a_y) and
//          becomes (cx, cy); at the end area += (r_x - cx) (cy - a_y) -- over the
//          kept points of w-rank < t and z-rank < s, in x order;
//   inner  V[t] = sum over s, ascending, of (z_s - z_{s-1}) A[t][s]
//          (z_{-1} = a_z, z_k = r_z);
//   outer  excl = sum over t, ascending, of (w_t - w_{t-1}) V[t]
//          (w_{-1} = a_w, w_k = r_w).
// All terms are >= 0: no subtraction of two volumes anywhere.
//
// Kernels (one stream, no cooperative launch, no workgroup waits on another)
//   k_hvx4_prep, k_hvx4_dom, k_hvx4_compact   tpe_mo_hvx.hip's three, restated
//                   for rows of four doubles: the rows that are not valid set to
//                   NaN, flag[i] = 1 for a row that a row of J weakly dominates,
//                   the live rows (flag 0) into a list
//   k_hvx4_excl     a fixed grid of workgroups, each taking live rows l, l +
//                   grid, ..: the kept set as in tpe_mo_hvx.hip, with 32-byte
//                   points (J in chunks of 256 rows, a thread a row: clip, drop
//                   what the kept set weakly dominates, append by ballot prefix,
//                   prune, compact through registers); three bitonic sorts of
//                   16-bit indices (w, z, (x, y)), the two rank arrays, and one
//                   8-byte record (index, w-rank, z-rank) per point in x order.
//                   Then the cells: a wave per outer slab t, the four waves
//                   striding over t = 0 .. k together; a lane per inner slab s,
//                   64 at a time.  Every lane of a wave reads the same record and
//                   the same point (LDS broadcasts) and differs only in the test
//                   z-rank < s; the test w-rank < t is the same for the whole
//                   wave.  The lanes' terms (z_s - z_{s-1}) A[t][s] go to the
//                   wave's line of 64 doubles, the wave adds them in ascending
//                   s -- batch after batch, so V[t] is one left-to-right sum --
//                   and lane 0 writes (w_t - w_{t-1}) V[t] to the workgroup's
//                   line; after the last t one thread adds that line in
//                   ascending t.  The loops over t and over the batches have the
//                   same trip counts in every wave (k is the workgroup's), so
//                   the barriers between writing and reading a line are reached
//                   by all.
// LDS of k_hvx4_excl, per workgroup: points (512 + 256) x 32 B = 24 576, the
// records 512 x 8 = 4 096, five index arrays 5 x 1 024, the waves' lines 4 x 64
// x 8 = 2 048, the workgroup's line 513 x 8 = 4 104, alive bytes 768, counters
// 1 056: 41.8 KB -- three workgroups on a CU's 160 KB.  A live row whose kept
// set exceeds the capacity after a prune gets NaN and counts in hdr[1]; the
// caller recomputes it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tpe_ctx.h"
#include "tpe_mo_hvx4.h"

namespace tpe_rt {

namespace {

constexpr int kM = 4;
constexpr int kHvx4Buf = kHvx4Cap + kBlock;       // the kept set plus one chunk's survivors
constexpr int kHvx4Per = kHvx4Buf / kBlock;       // entries a thread moves in a compaction
constexpr int kHvx4Waves = kBlock / 64;
constexpr unsigned kHvx4Pad = 0xFFFFu;            // index of a padding slot of a sort: past every point
constexpr unsigned kHvx4Grid = 768;               // workgroups of k_hvx4_excl: 3 per CU
static_assert(kHvx4Buf % kBlock == 0, "a thread moves whole entries");
static_assert((kHvx4Cap & (kHvx4Cap - 1)) == 0 && kHvx4Cap >= 256 && kHvx4Cap < (int)kHvx4Pad,
              "the sorts pad to a power of two within the index arrays");

struct alignas(8) Hvx4Rec {   // one 8-byte LDS read
    uint16_t e, wr, zr, pad;  // a kept point, its w-rank, its z-rank
};

__global__ __launch_bounds__(kBlock) void k_hvx4_prep(double* __restrict__ F, int32_t n, Hvx4Ref ref,
                                                      int32_t* __restrict__ flag, int32_t* __restrict__ hdr,
                                                      double* __restrict__ excl) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i == 0)
        for (int q = 0; q < kHvx4Hdr; ++q) hdr[q] = 0;
    if (i >= n) return;
    bool ok = true;
#pragma unroll
    for (int m = 0; m < kM; ++m) {
        const double f = F[(size_t)i * kM + m];
        ok &= f > -__builtin_inf() && f < ref.r[m];   // (a NaN fails both)
    }
    if (!ok)
#pragma unroll
        for (int m = 0; m < kM; ++m) F[(size_t)i * kM + m] = __builtin_nan("");
    flag[i] = ok ? 0 : 2;
    excl[i] = 0.0;
}

__global__ __launch_bounds__(kBlock) void k_hvx4_dom(const double* __restrict__ F, int32_t n, int32_t per_slice,
                                                     int32_t mode, int32_t* __restrict__ flag) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    // a lane past the rows, and a row that is not valid, compares NaNs: never dominated
    double fi[kM];
#pragma unroll
    for (int m = 0; m < kM; ++m) fi[m] = i < n ? F[(size_t)i * kM + m] : __builtin_nan("");
    const int32_t j0 = (int32_t)blockIdx.y * per_slice;          // (uniform over the workgroup)
    int32_t j1 = min(n, j0 + per_slice);
    if (mode == 0) j1 = min(j1, (int32_t)((blockIdx.x + 1) * kBlock));   // no row of the block has a later j
    bool dom = false;
#pragma unroll 4
    for (int32_t j = j0; j < j1; ++j) {
        const double* __restrict__ fj = F + (size_t)j * kM;
        bool le = true;
#pragma unroll
        for (int m = 0; m < kM; ++m) le &= fj[m] <= fi[m];
        dom |= le && (mode == 0 ? j < i : j != i);
    }
    if (dom && i < n) flag[i] = 1;   // (every writer writes 1)
}

__global__ __launch_bounds__(kBlock) void k_hvx4_compact(const int32_t* __restrict__ flag, int32_t n,
                                                         int32_t* __restrict__ live, int32_t* __restrict__ hdr) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const bool is_live = i < n && flag[i] == 0;
    const unsigned long long bal = __ballot(is_live);
    const int lane = (int)(threadIdx.x & 63);
    int32_t base = 0;
    if (lane == 0 && bal) base = atomicAdd(hdr, (int32_t)__popcll(bal));
    base = __shfl(base, 0, 64);
    if (is_live) live[base + (int32_t)__popcll(bal & (((unsigned long long)1 << lane) - 1))] = i;   // < n
}

// ia before ib by axis A, then axis B (B < 0: none), then index; padding last
template <int A, int B>
__device__ inline bool hvx4_before(const double* pts, unsigned ia, unsigned ib) {
    if (ia == kHvx4Pad) return false;
    if (ib == kHvx4Pad) return true;
    const double ka = pts[ia * kM + A], kb = pts[ib * kM + A];
    if (ka != kb) return ka < kb;
    if (B >= 0) {
        const double la = pts[ia * kM + (B >= 0 ? B : 0)], lb = pts[ib * kM + (B >= 0 ? B : 0)];
        if (la != lb) return la < lb;
    }
    return ia < ib;
}

// ord[0 .. np), np a power of two <= kHvx4Cap: the indices k .. np - 1 are
// padding.  Ends with a barrier.
template <int A, int B>
__device__ inline void hvx4_sort(const double* pts, uint16_t* ord, int k, int np) {
    for (int e = (int)threadIdx.x; e < np; e += kBlock) ord[e] = (uint16_t)(e < k ? (unsigned)e : kHvx4Pad);
    __syncthreads();
    for (int size = 2; size <= np; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = (int)threadIdx.x; t < (np >> 1); t += kBlock) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;   // hi < np
                const bool up = (lo & size) == 0;
                const unsigned x = ord[lo], y = ord[hi];
                if (hvx4_before<A, B>(pts, y, x) == up) {
                    ord[lo] = (uint16_t)y;
                    ord[hi] = (uint16_t)x;
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(kBlock) void k_hvx4_excl(const double* __restrict__ F, int32_t n, Hvx4Ref ref,
                                                      int32_t mode, int32_t cap, const int32_t* __restrict__ live,
                                                      int32_t* __restrict__ hdr, double* __restrict__ excl) {
    __shared__ double pts[kHvx4Buf * kM];
    __shared__ double sline[kHvx4Waves][64];      // a wave's terms of one batch of inner slabs
    __shared__ double tline[kHvx4Cap + 1];        // the outer slabs' terms
    __shared__ Hvx4Rec xrec[kHvx4Cap];            // the points in x order
    __shared__ uint16_t word[kHvx4Cap], zord[kHvx4Cap], xord[kHvx4Cap], wrank[kHvx4Cap], zrank[kHvx4Cap];
    __shared__ unsigned char alive[kHvx4Buf];
    __shared__ int32_t cnt[kBlock];
    __shared__ int32_t wtot[2][kHvx4Waves];
    const int T = (int)threadIdx.x, lane = T & 63, w = T >> 6;
    const int32_t n_live = min(hdr[0], n);
    for (int32_t l = (int32_t)blockIdx.x; l < n_live; l += (int32_t)gridDim.x) {
        const int32_t i = live[l];
        double a[kM];
#pragma unroll
        for (int m = 0; m < kM; ++m) a[m] = F[(size_t)i * kM + m];
        const int32_t jend = mode == 0 ? i : n;
        int k = 0;                 // the kept set pts[0 .. k): the same value in every thread
        bool over = false;
        int par = 0;
        for (int32_t j0 = 0; j0 < jend; j0 += kBlock, par ^= 1) {
            const int32_t j = j0 + T;
            bool have = j < jend && j != i;
            double c[kM];
#pragma unroll
            for (int m = 0; m < kM; ++m) {
                const double f = have ? F[(size_t)j * kM + m] : __builtin_nan("");
                have = have && f < ref.r[m];          // (a row that is not valid is NaN)
                c[m] = f > a[m] ? f : a[m];
            }
            for (int e = 0; have && e < k; ++e) {     // weakly dominated by a kept point: gone
                bool le = true;
#pragma unroll
                for (int m = 0; m < kM; ++m) le &= pts[e * kM + m] <= c[m];
                have = !le;
            }
            const unsigned long long bal = __ballot(have);
            if (lane == 0) wtot[par][w] = (int32_t)__popcll(bal);
            __syncthreads();
            int ns = 0, base = 0;
#pragma unroll
            for (int q = 0; q < kHvx4Waves; ++q) {
                const int v = wtot[par][q];
                base += q < w ? v : 0;
                ns += v;
            }
            if (ns == 0) continue;                    // (uniform; wtot[par] is rewritten two barriers on at the earliest)
            // the survivors behind the kept set: k + ns <= cap + 256 <= kHvx4Buf entries
            if (have) {
                const int pos = k + base + (int)__popcll(bal & (((unsigned long long)1 << lane) - 1));
#pragma unroll
                for (int m = 0; m < kM; ++m) pts[pos * kM + m] = c[m];
            }
            __syncthreads();
            const int tot = k + ns;
            // an entry dies when a new point lies weakly below it (equal points: the later one)
            for (int e = T; e < tot; e += kBlock) {
                double p[kM];
#pragma unroll
                for (int m = 0; m < kM; ++m) p[m] = pts[e * kM + m];
                bool dead = false;
                for (int q = k; q < tot && !dead; ++q) {
                    bool le = true, lt = false;
#pragma unroll
                    for (int m = 0; m < kM; ++m) {
                        const double v = pts[q * kM + m];
                        le &= v <= p[m];
                        lt |= v < p[m];
                    }
                    dead = q != e && le && (lt || q < e);
                }
                alive[e] = dead ? 0 : 1;
            }
            __syncthreads();
            // stable compaction: a thread holds kHvx4Per consecutive entries in registers
            double reg[kHvx4Per][kM];
            bool ok[kHvx4Per];
            int mine = 0;
#pragma unroll
            for (int u = 0; u < kHvx4Per; ++u) {
                const int e = T * kHvx4Per + u;       // < kHvx4Buf
                ok[u] = e < tot && alive[e];
#pragma unroll
                for (int m = 0; m < kM; ++m) reg[u][m] = ok[u] ? pts[e * kM + m] : 0.0;
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
            for (int u = 0; u < kHvx4Per; ++u)
                if (ok[u]) {                          // off < total <= tot <= kHvx4Buf
#pragma unroll
                    for (int m = 0; m < kM; ++m) pts[off * kM + m] = reg[u][m];
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
        // k <= cap <= kHvx4Cap
        int np = 1;
        while (np < k) np <<= 1;
        hvx4_sort<3, -1>(pts, word, k, np);
        hvx4_sort<2, -1>(pts, zord, k, np);
        hvx4_sort<0, 1>(pts, xord, k, np);
        for (int p = T; p < k; p += kBlock) {         // word[p], zord[p] < k
            wrank[word[p]] = (uint16_t)p;
            zrank[zord[p]] = (uint16_t)p;
        }
        __syncthreads();
        for (int p = T; p < k; p += kBlock) {
            const unsigned e = xord[p];               // < k
            xrec[p] = Hvx4Rec{(uint16_t)e, wrank[e], zrank[e], 0};
        }
        __syncthreads();
        // the cells: wave w takes the outer slabs t = w, w + 4, ..; its lanes the inner slabs
        const int nbatch = (k + 64) / 64;             // batches of 64 inner slabs s = 0 .. k
        const double a_z = a[2], a_w = a[3], r_z = ref.r[2], r_w = ref.r[3];   // (values, not addresses, below)
        for (int t0 = 0; t0 <= k; t0 += kHvx4Waves) {
            const int t = t0 + w;                     // (t > k: the wave only keeps the barriers)
            double V = 0.0;
            for (int q = 0; q < nbatch; ++q) {
                const int s = q * 64 + lane;
                if (t <= k && s <= k) {
                    double cx = a[0], cy = ref.r[1], area = 0.0;
                    for (int p = 0; p < k; ++p) {
                        const Hvx4Rec rec = xrec[p];
                        if ((int)rec.wr >= t) continue;            // (the same in every lane of the wave)
                        const double y = pts[rec.e * kM + 1];
                        if ((int)rec.zr < s && y < cy) {
                            const double x = pts[rec.e * kM];
                            area = area + (x - cx) * (cy - a[1]);
                            cx = x;
                            cy = y;
                        }
                    }
                    area = area + (ref.r[0] - cx) * (cy - a[1]);
                    const double lo = s == 0 ? a_z : pts[zord[s - 1] * kM + 2];
                    const double hi = s == k ? r_z : pts[zord[s] * kM + 2];
                    sline[w][lane] = (hi - lo) * area;
                }
                __syncthreads();
                if (t <= k) {                         // every lane the same sum, left to right
                    const int m = min(64, k + 1 - q * 64);
                    for (int u = 0; u < m; ++u) V = q == 0 && u == 0 ? sline[w][0] : V + sline[w][u];
                }
                __syncthreads();
            }
            if (lane == 0 && t <= k) {
                const double lo = t == 0 ? a_w : pts[word[t - 1] * kM + 3];
                const double hi = t == k ? r_w : pts[word[t] * kM + 3];
                tline[t] = (hi - lo) * V;
            }
        }
        __syncthreads();
        if (T == 0) {
            double v = tline[0];
            for (int t = 1; t <= k; ++t) v = v + tline[t];
            excl[i] = v;
        }
        __syncthreads();
    }
}

}  // namespace

void hvx4_launch(hipStream_t st, double* F, int32_t n, Hvx4Ref ref, int32_t mode, int32_t cap, dim3 pair_grid,
                 int32_t per_slice, int32_t* flag, int32_t* live, int32_t* hdr, double* excl) {
    cap = std::max(1, std::min(cap, kHvx4Cap));
    const dim3 rows((unsigned)((n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_hvx4_prep, rows, dim3(kBlock), 0, st, F, n, ref, flag, hdr, excl);
    hipLaunchKernelGGL(k_hvx4_dom, pair_grid, dim3(kBlock), 0, st, F, n, per_slice, mode, flag);
    hipLaunchKernelGGL(k_hvx4_compact, rows, dim3(kBlock), 0, st, flag, n, live, hdr);
    hipLaunchKernelGGL(k_hvx4_excl, dim3(std::min<unsigned>(kHvx4Grid, (unsigned)n)), dim3(kBlock), 0, st, F, n, ref,
                       mode, cap, live, hdr, excl);
}

}  // namespace tpe_rt
