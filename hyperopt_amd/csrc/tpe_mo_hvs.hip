// tpe_mo_hvs.hip -- the sampled hypervolume tie-break of the below set, two to
// eight objectives (include/hyperopt_tpe.h, tpe_mo_keys_hvs): greedy subset
// selection inside the level that straddles position n_select, with the gain
// of a row counted on a fixed set of sample points (HypE, Bader & Zitzler).
//
// Coordinates.  r[i][m] = the rank rows j with F[j][m] < F[i][m], n_f rank
// rows, every box [r[i], n_f).  lo[m] = the level's smallest rank on axis m,
// span[m] = n_f - lo[m] >= 1: [lo, n_f) bounds the union of the level's boxes.
// Sample s = 0 .. S - 1 has x[s][m] = lo[m] + ((uint64)word * span[m] >> 32),
// word = word m % 4 of philox4x32_10 with counter (s, m / 4, 0,
// TPE_MO_HVS_STREAM) under the key (TPE_MO_HVS_KEY0, TPE_MO_HVS_KEY1).  Row c
// covers s iff r[c][m] <= x[s][m] on every axis; gain(c | P) = the samples c
// covers and no row of P covers -- integers throughout.
//
// Kernels (the first three restate tpe_mo_hv.hip's for up to eight columns)
//   k_hvs_pairs<M>   k_mo_pairs<M> (tpe_mo.hip) with M more counters, fj[m] <
//                    fi[m]; one integer atomicAdd per counter and slice
//   k_hvs_find       a thread per sorted position: the level's start a, its
//                    end, q = n_select - a and n_f, each written by the one
//                    thread on that boundary; all 0 when no level straddles
//   k_hvs_compact    the level's rows (row, do, ranks) gathered to t = p - a
//   -- the host reads the header here: L, q, n_f --
//   k_hvs_lo         a workgroup per axis: the minimum of the level's ranks
//   k_hvs_points     a thread per (sample, block of four axes): one Philox call,
//                    up to four coordinates, stored axis-major (pts[m][s])
//   k_hvs_cover<M>   a wave per (word of 64 samples, tile of candidates): lane l
//                    holds sample 64 w + l in M VGPRs; the candidates' ranks
//                    come by wave-uniform loads (the scalar cache); the ballot
//                    of "every x[m] >= r[m]" IS the 64-bit word of (candidate,
//                    w); lane j keeps candidate c0 + j's and the 64 words leave
//                    as one coalesced store: bits[w][c], candidate-contiguous
//   per pick:
//   k_hvs_gain       grid (candidate blocks, word chunks): a thread holds one
//                    candidate and adds popcount(bits[w][c] & ~covered[w]) over
//                    its chunk -- bits coalesced, covered[w] wave-uniform --
//                    then one integer atomicAdd into cgain[c]
//   k_hvs_pick       one workgroup: (gain, do, smaller row) over the unpicked
//                    rows by wave shuffles, then LDS slots; writes the pick and
//                    its gain, flags the row, ORs its words into covered and
//                    zeroes cgain for the next pick
//   k_hvs_tail       the level's keys: the picks from a in pick order, the
//                    others behind them in their old order
// No workgroup waits on another, nothing is launched cooperatively and the
// host does not synchronise between picks.
#include <hip/hip_runtime.h>

#include "../../include/hyperopt_tpe.h"
#include "tpe_ctx.h"
#include "tpe_device.h"
#include "tpe_mo_hvs.h"

namespace tpe_rt {

namespace {

typedef unsigned long long u64;

constexpr int kPick = 1024;                 // k_hvs_pick's workgroup
constexpr int kPickWaves = kPick / 64;
constexpr int kCoverWaves = kBlock / 64;    // words of one k_hvs_cover workgroup
constexpr int kCoverTile = 256;             // candidates of one k_hvs_cover workgroup: 4 stores a wave
constexpr unsigned kGainBlocks = 1024;      // workgroups wanted of k_hvs_gain: 4 per CU

template <int M>
__global__ __launch_bounds__(kBlock) void k_hvs_pairs(const double* __restrict__ F, int32_t n, int32_t per_slice,
                                                      int32_t* __restrict__ by, int32_t* __restrict__ dom,
                                                      uint32_t* __restrict__ rank) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    // a lane past the rows compares NaNs: every test below is false for it
    double fi[M];
#pragma unroll
    for (int m = 0; m < M; ++m) fi[m] = i < n ? F[(size_t)i * M + m] : __builtin_nan("");
    const int32_t j0 = (int32_t)blockIdx.y * per_slice;          // (uniform over the workgroup)
    const int32_t j1 = min(n, j0 + per_slice);
    int32_t n_by = 0, n_do = 0;
    uint32_t n_lt[M];
#pragma unroll
    for (int m = 0; m < M; ++m) n_lt[m] = 0;
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
            n_lt[m] += v < fi[m] ? 1u : 0u;      // (a NaN on either side: not counted)
        }
        n_do += (le && !ge) ? 1 : 0;
        n_by += (ge && !le) ? 1 : 0;
    }
    if (i < n) {
        if (n_by) atomicAdd(by + i, n_by);
        if (n_do) atomicAdd(dom + i, n_do);
#pragma unroll
        for (int m = 0; m < M; ++m)
            if (n_lt[m]) atomicAdd(rank + (size_t)m * n + i, n_lt[m]);
    }
}

// 0 < n_select < n.  A position's row is a rank row when it has a key (by
// field != n) and, with constraints, is feasible; the rank rows are a prefix of
// the order.  Inactive (the header is 0, the keys stay): the rows at n_select -
// 1 and n_select differ in by, or one of them is no rank row.
__global__ __launch_bounds__(kBlock) void k_hvs_find(const uint64_t* __restrict__ sorted, int32_t n, int32_t bits,
                                                     const double* __restrict__ v, int32_t n_select,
                                                     int32_t* __restrict__ hdr) {
    const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const uint64_t mask = ((uint64_t)1 << bits) - 1;
    auto by_of = [&](int32_t at) { return (int64_t)(sorted[at] >> (2 * bits)); };
    auto ranked = [&](int32_t at) {
        const uint64_t k = sorted[at];
        if ((int64_t)(k >> (2 * bits)) == n) return false;
        return !v || v[(int32_t)(k & mask)] == 0.0;
    };
    const int64_t bs = by_of(n_select - 1);
    const bool active = bs == by_of(n_select) && ranked(n_select - 1) && ranked(n_select);
    if (!active) {
        if (p == 0) hdr[0] = hdr[1] = hdr[2] = hdr[3] = 0;
        return;
    }
    if (p >= n) return;
    if (ranked(p) && (p == n - 1 || !ranked(p + 1))) hdr[3] = p + 1;
    if (by_of(p) != bs) return;
    if (p == 0 || by_of(p - 1) != bs) {
        hdr[0] = p;
        hdr[2] = n_select - p;
    }
    if (p == n - 1 || by_of(p + 1) != bs) hdr[1] = p + 1;
}

__global__ __launch_bounds__(kBlock) void k_hvs_compact(const uint64_t* __restrict__ sorted, int32_t n, int32_t bits,
                                                        int32_t n_obj, const uint32_t* __restrict__ rank,
                                                        const int32_t* __restrict__ hdr, int32_t* __restrict__ lvl,
                                                        uint32_t* __restrict__ lvl_r,
                                                        unsigned char* __restrict__ flag) {
    const int32_t p = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const int32_t a = hdr[0], end = hdr[1];
    if (p < a || p >= end || p >= n) return;
    const uint64_t mask = ((uint64_t)1 << bits) - 1;
    const uint64_t k = sorted[p];
    const int32_t i = (int32_t)(k & mask), t = p - a;
    lvl[t] = i;
    lvl[(size_t)n + t] = n - (int32_t)((k >> bits) & mask);
    for (int m = 0; m < n_obj; ++m) lvl_r[(size_t)m * n + t] = rank[(size_t)m * n + i];
    flag[t] = 0;
}

// lo[m], m = blockIdx.x: wave shuffles, then one LDS slot a wave
__global__ __launch_bounds__(kBlock) void k_hvs_lo(const uint32_t* __restrict__ lvl_r, int32_t n, int32_t L,
                                                   uint32_t* __restrict__ lo) {
    __shared__ uint32_t slot[kBlock / 64];
    const uint32_t* r = lvl_r + (size_t)blockIdx.x * n;
    uint32_t best = 0xFFFFFFFFu;
    for (int32_t t = (int32_t)threadIdx.x; t < L; t += kBlock) best = min(best, r[t]);
#pragma unroll
    for (int o = 32; o; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o));
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) best = min(best, slot[w]);
        lo[blockIdx.x] = best;
    }
}

// pts[m][s] for the axes 4 blockIdx.y .. 4 blockIdx.y + 3 below M
__global__ __launch_bounds__(kBlock) void k_hvs_points(const uint32_t* __restrict__ lo, int32_t M, int32_t S,
                                                       uint32_t n_f, uint32_t* __restrict__ pts) {
    const int32_t s = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (s >= S) return;
    const uint32_t blk = blockIdx.y;
    const tpe::U4 w = tpe::philox4x32_10(tpe::U4{(uint32_t)s, blk, 0u, (uint32_t)TPE_MO_HVS_STREAM},
                                         (uint32_t)TPE_MO_HVS_KEY0, (uint32_t)TPE_MO_HVS_KEY1);
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t m = (int32_t)blk * 4 + k;
        if (m < M) {
            const uint32_t l = lo[m];
            pts[(size_t)m * S + s] = l + (uint32_t)(((uint64_t)word[k] * (uint64_t)(n_f - l)) >> 32);
        }
    }
}

// bits[w][c]: wave `wave` of workgroup (bx, by) has the word w = kCoverWaves bx
// + wave and the candidates kCoverTile by .. + kCoverTile - 1 below L.  The
// candidate index is uniform over the workgroup, so its ranks are scalar loads.
template <int M>
__global__ __launch_bounds__(kBlock) void k_hvs_cover(const uint32_t* __restrict__ pts,
                                                      const uint32_t* __restrict__ lvl_r, int32_t n, int32_t L,
                                                      int32_t S, uint64_t* __restrict__ bits) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int32_t w = (int32_t)blockIdx.x * kCoverWaves + ((int32_t)threadIdx.x >> 6);
    if (w >= (S >> 6)) return;                       // (uniform over the wave; the kernel has no barrier)
    uint32_t x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = pts[(size_t)m * S + (size_t)w * 64 + lane];
    const int32_t tile0 = (int32_t)blockIdx.y * kCoverTile;
    for (int32_t c0 = tile0; c0 < min(L, tile0 + kCoverTile); c0 += 64) {
        const int32_t cn = min(64, L - c0);
        uint64_t mine = 0;
        for (int32_t j = 0; j < cn; ++j) {
            bool in = true;
#pragma unroll
            for (int m = 0; m < M; ++m) in &= x[m] >= lvl_r[(size_t)m * n + c0 + j];
            const uint64_t word = __ballot(in);
            if (lane == j) mine = word;
        }
        if (lane < cn) bits[(size_t)w * L + c0 + lane] = mine;
    }
}

// cgain[c] += the samples of the words w0 .. w0 + per_chunk - 1 that c covers
// and P does not
__global__ __launch_bounds__(kBlock) void k_hvs_gain(const uint64_t* __restrict__ bits,
                                                     const uint64_t* __restrict__ covered, int32_t L, int32_t W,
                                                     int32_t per_chunk, uint32_t* __restrict__ cgain) {
    const int32_t c = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    const int32_t w0 = (int32_t)blockIdx.y * per_chunk, w1 = min(W, w0 + per_chunk);
    if (c >= L) return;
    uint32_t g = 0;
#pragma unroll 4
    for (int32_t w = w0; w < w1; ++w) g += (uint32_t)__popcll(bits[(size_t)w * L + c] & ~covered[w]);
    if (g) atomicAdd(cgain + c, g);
}

// larger gain, then larger do, then smaller row: tie = do << 32 | ~row, never 0
// for a row, 0 (with gain 0, t -1) for a thread without one
struct Cand {
    u64 tie;
    uint32_t gain;
    int32_t t;
};

__device__ inline bool better(const Cand& x, const Cand& y) {
    return x.gain > y.gain || (x.gain == y.gain && x.tie > y.tie);
}

// the best of the wave, in every lane (ties are distinct among rows)
__device__ inline Cand wave_best(Cand c) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        Cand d;
        d.tie = __shfl_xor(c.tie, o);
        d.gain = (uint32_t)__shfl_xor((int)c.gain, o);
        d.t = __shfl_xor(c.t, o);
        if (better(d, c)) c = d;
    }
    return c;
}

// pick number cnt (the host enqueues q < L of them: an unpicked row exists)
__global__ __launch_bounds__(kPick) void k_hvs_pick(const int32_t* __restrict__ lvl, int32_t n, int32_t L, int32_t W,
                                                    int32_t cnt, const uint64_t* __restrict__ bits,
                                                    uint32_t* __restrict__ cgain, unsigned char* __restrict__ flag,
                                                    uint64_t* __restrict__ covered, int32_t* __restrict__ pick,
                                                    int32_t* __restrict__ pick_t, u64* __restrict__ gain) {
    __shared__ u64 slot_tie[kPickWaves];
    __shared__ uint32_t slot_gain[kPickWaves];
    __shared__ int32_t slot_t[kPickWaves];
    __shared__ int32_t won;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* lvl_do = lvl + n;
    Cand best{0, 0, -1};
    for (int32_t t = tid; t < L; t += kPick) {
        const uint32_t g = cgain[t];
        cgain[t] = 0;                                  // (read by this thread alone: ready for the next pick)
        if (flag[t]) continue;
        Cand me;
        me.gain = g;
        me.tie = ((u64)(uint32_t)lvl_do[t] << 32) | (u64)(uint32_t)~(uint32_t)lvl[t];
        me.t = t;
        if (better(me, best)) best = me;
    }
    best = wave_best(best);
    if (lane == 0) {
        slot_tie[wave] = best.tie;
        slot_gain[wave] = best.gain;
        slot_t[wave] = best.t;
    }
    __syncthreads();
    if (wave == 0) {
        Cand w{0, 0, -1};
        if (lane < kPickWaves) {
            w.tie = slot_tie[lane];
            w.gain = slot_gain[lane];
            w.t = slot_t[lane];
        }
        w = wave_best(w);
        if (lane == 0) {
            won = w.t;
            if (w.t >= 0) {
                pick[cnt] = lvl[w.t];
                pick_t[cnt] = w.t;
                gain[cnt] = (u64)w.gain;
                flag[w.t] = 1;
            }
        }
    }
    __syncthreads();
    const int32_t t = won;
    if (t < 0) return;                                 // (uniform; not reached for cnt < q < L)
    for (int32_t w = tid; w < W; w += kPick) covered[w] |= bits[(size_t)w * L + t];
}

// the level's keys: the picks from a in pick order, the others behind them
__global__ __launch_bounds__(kBlock) void k_hvs_tail(const int32_t* __restrict__ lvl, int32_t L, int32_t a, int32_t q,
                                                     const unsigned char* __restrict__ flag,
                                                     const int32_t* __restrict__ pick_t, double* __restrict__ keys) {
    const int32_t t = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (t >= L) return;
    int32_t before = 0, at = -1;
    for (int k = 0; k < q; ++k) {
        const int32_t pt = pick_t[k];                  // (uniform: scalar loads)
        before += pt < t ? 1 : 0;
        if (pt == t) at = k;
    }
    keys[lvl[t]] = flag[t] ? (double)(a + at) : (double)(a + q + t - before);
}

template <int M>
void launch_cover(dim3 grid, hipStream_t st, const HvsBufs& b, int32_t n, int32_t L, int32_t S) {
    hipLaunchKernelGGL(k_hvs_cover<M>, grid, dim3(kBlock), 0, st, b.pts, b.lvl_r, n, L, S, b.bits);
}

}  // namespace

void hvs_launch_pairs(int32_t n_obj, dim3 grid, hipStream_t st, const double* F, int32_t n, int32_t per_slice,
                      int32_t* by, int32_t* dom, uint32_t* rank) {
#define HVS_PAIRS(M) \
    case M: hipLaunchKernelGGL(k_hvs_pairs<M>, grid, dim3(kBlock), 0, st, F, n, per_slice, by, dom, rank); break
    switch (n_obj) {
        HVS_PAIRS(2);
        HVS_PAIRS(3);
        HVS_PAIRS(4);
        HVS_PAIRS(5);
        HVS_PAIRS(6);
        HVS_PAIRS(7);
        HVS_PAIRS(8);
        default: break;                                // (refused by the caller)
    }
#undef HVS_PAIRS
}

void hvs_launch_level(int32_t n_obj, hipStream_t st, const HvsBufs& b, int32_t n, int32_t bits, int32_t n_select) {
    const dim3 rows((unsigned)((n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_hvs_find, rows, dim3(kBlock), 0, st, b.sorted, n, bits, b.v, n_select, b.hdr);
    hipLaunchKernelGGL(k_hvs_compact, rows, dim3(kBlock), 0, st, b.sorted, n, bits, n_obj, b.rank, b.hdr, b.lvl,
                       b.lvl_r, b.flag);
}

void hvs_launch_select(int32_t n_obj, hipStream_t st, const HvsBufs& b, int32_t n, int32_t a, int32_t L, int32_t q,
                       int32_t n_f, int32_t n_samples) {
    const int32_t S = n_samples, W = S / 64;
    hipLaunchKernelGGL(k_hvs_lo, dim3((unsigned)n_obj), dim3(kBlock), 0, st, b.lvl_r, n, L, b.lo);
    hipLaunchKernelGGL(k_hvs_points, dim3((unsigned)((S + kBlock - 1) / kBlock), (unsigned)((n_obj + 3) / 4)),
                       dim3(kBlock), 0, st, b.lo, n_obj, S, (uint32_t)n_f, b.pts);
    const dim3 cgrid((unsigned)((W + kCoverWaves - 1) / kCoverWaves), (unsigned)((L + kCoverTile - 1) / kCoverTile));
    switch (n_obj) {
        case 2: launch_cover<2>(cgrid, st, b, n, L, S); break;
        case 3: launch_cover<3>(cgrid, st, b, n, L, S); break;
        case 4: launch_cover<4>(cgrid, st, b, n, L, S); break;
        case 5: launch_cover<5>(cgrid, st, b, n, L, S); break;
        case 6: launch_cover<6>(cgrid, st, b, n, L, S); break;
        case 7: launch_cover<7>(cgrid, st, b, n, L, S); break;
        default: launch_cover<8>(cgrid, st, b, n, L, S); break;
    }
    // candidate blocks x word chunks: enough workgroups for the chip
    const unsigned cblocks = (unsigned)((L + kBlock - 1) / kBlock);
    const unsigned chunks = std::max(1u, std::min((unsigned)W, kGainBlocks / cblocks));
    const int32_t per_chunk = (int32_t)((W + chunks - 1) / chunks);
    const dim3 ggrid(cblocks, (unsigned)((W + per_chunk - 1) / per_chunk));
    for (int32_t cnt = 0; cnt < q; ++cnt) {
        hipLaunchKernelGGL(k_hvs_gain, ggrid, dim3(kBlock), 0, st, b.bits, b.covered, L, W, per_chunk, b.cgain);
        hipLaunchKernelGGL(k_hvs_pick, dim3(1), dim3(kPick), 0, st, b.lvl, n, L, W, cnt, b.bits, b.cgain, b.flag,
                           b.covered, b.pick, b.pick_t, b.gain);
    }
    hipLaunchKernelGGL(k_hvs_tail, dim3(cblocks), dim3(kBlock), 0, st, b.lvl, L, a, q, b.flag, b.pick_t, b.keys);
}

}  // namespace tpe_rt
