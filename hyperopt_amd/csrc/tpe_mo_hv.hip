// tpe_mo_hv.hip -- the hypervolume tie-break of the below set
// (include/hyperopt_tpe.h, tpe_mo_keys_hv): greedy hypervolume subset
// selection inside the level of equal dominated_by that straddles position
// n_select of tpe_mo_keys' order.
//
// Coordinates.  r[i][m] = the rank rows j with F[j][m] < F[i][m] (rank rows:
// the rows of the dominance pass, n_f of them); the reference point is n_f on
// every axis, so row i's box has the sides s[i][m] = n_f - r[i][m] >= 1.  The
// kernels below work on the sides: a box is [0, s0) x [0, s1) (x [0, s2)),
// anchored at the origin, the clipped point max(c, p) of the rank coordinates
// is min(c, p) of the sides, and a volume is a count of integer cells -- an
// exact unsigned 64-bit integer below 2^60 (n <= 2^20, three axes).
//
// Kernels
//   k_hv_prep       (no constraints) a row with a NaN: NaN in every objective
//   k_hv_pairs<M>   k_mo_pairs<M> (tpe_mo.hip: the same scalar-load walk over
//                   the j-slice) with M more counters, fj[m] < fi[m]; one
//                   integer atomicAdd per counter and slice
//   k_hv_find       a thread per sorted position: whether a feasible level
//                   straddles n_select, and its start a, its end, q = n_select
//                   - a and n_f -- each written by the one thread that sits on
//                   that boundary, so no atomics and no second pass
//   k_hv_compact    the level's rows (row, do, ranks) gathered to t = p - a
//   k_hv_select<M>  one workgroup of 1024 threads, the level strided over
//                   them.  The picked set P (at most 64 rows) lives in LDS,
//                   sorted by descending s0 (M = 2: ascending r0) or
//                   descending s2 (M = 3: ascending r2).  Per pick every
//                   thread evaluates gain(c) = vol(c) - covered(c) of its
//                   rows, the waves reduce (gain, do, smaller row) by
//                   shuffles, 16 slots in LDS, barrier, wave 0 reduces the
//                   slots, writes the pick, flags it and inserts it, barrier.
//                   covered(c), the union of the boxes min(c, p):
//                   M = 2   the level is an antichain, so along P s0 falls and
//                           s1 rises, and clipping keeps that: one pass,
//                           sum (w_j - w_j+1) h_j
//                   M = 3   slabs along s2: between the clipped depths d_j and
//                           d_j+1 the cross-section is the 2-D union of P's
//                           first j + 1 rows clipped by c -- and that is the
//                           unclipped union cut by c's rectangle, so the
//                           staircase of every prefix of P is kept ONCE, in
//                           LDS, for all threads (64 * 65 / 2 corners, two
//                           copies: wave 0 writes the next pick's while the
//                           old one is its input), not per thread.  Lane j of
//                           wave 0 rebuilds prefix j: the old prefix j - 1
//                           plus the pick, one pass.  A thread reads a
//                           staircase at one address per wave: LDS broadcasts.
//                   The tail rewrites the keys of the level's rows: the picks
//                   in pick order from a, the others behind them in their old
//                   order.
#include <hip/hip_runtime.h>

#include "tpe_ctx.h"
#include "tpe_mo_hv.h"

namespace tpe_rt {

namespace {

typedef unsigned long long u64;

constexpr int kSel = 1024;
constexpr int kSelWaves = kSel / 64;
constexpr int kStair = kHvMaxPicks * (kHvMaxPicks + 1) / 2;   // corners of all the prefixes' staircases

template <int M>
__global__ __launch_bounds__(kBlock) void k_hv_pairs(const double* __restrict__ F, int32_t n, int32_t per_slice,
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
#pragma unroll 4
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

// without constraints: NaN over the whole row of a row with a NaN, in place on
// the device copy -- such a row is no rank row, and its other values may not be
// counted by k_hv_pairs (with constraints k_moc_prep has done so)
__global__ __launch_bounds__(kBlock) void k_hv_prep(double* __restrict__ F, int32_t n, int32_t n_obj) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    bool nan = false;
    for (int m = 0; m < n_obj; ++m) {
        const double f = F[(size_t)i * n_obj + m];
        nan |= f != f;
    }
    if (nan)
        for (int m = 0; m < n_obj; ++m) F[(size_t)i * n_obj + m] = __builtin_nan("");
}

// 0 < n_select < n.  A position's row is a rank row when it has a key (by
// field != n) and, with constraints, is feasible; the rank rows are a prefix of
// the order.  Inactive (the keys stay): the rows at n_select - 1 and n_select
// differ in by, or one of them is no rank row.
__global__ __launch_bounds__(kBlock) void k_hv_find(const uint64_t* __restrict__ sorted, int32_t n, int32_t bits,
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

template <int M>
__global__ __launch_bounds__(kBlock) void k_hv_compact(const uint64_t* __restrict__ sorted, int32_t n, int32_t bits,
                                                       const uint32_t* __restrict__ rank,
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
#pragma unroll
    for (int m = 0; m < M; ++m) lvl_r[(size_t)m * n + t] = rank[(size_t)m * n + i];
    flag[t] = 0;
}

// larger gain, then larger do, then smaller row: tie = do << 32 | ~row, never 0
// for a row, 0 (with gain 0, t -1) for a thread without one
struct Cand {
    u64 gain, tie;
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
        d.gain = __shfl_xor(c.gain, o);
        d.tie = __shfl_xor(c.tie, o);
        d.t = __shfl_xor(c.t, o);
        if (better(d, c)) c = d;
    }
    return c;
}

template <int M>
__global__ __launch_bounds__(kSel) void k_hv_select(const int32_t* __restrict__ hdr, const int32_t* __restrict__ lvl,
                                                    const uint32_t* __restrict__ lvl_r,
                                                    unsigned char* flag, int32_t n,
                                                    double* __restrict__ keys, int32_t* __restrict__ pick,
                                                    u64* __restrict__ gain) {
    __shared__ uint32_t ps[M][kHvMaxPicks];            // P's sides, sorted by descending ps[M - 1] (M = 2: ps[0])
    __shared__ int32_t pick_t[kHvMaxPicks], pick_i[kHvMaxPicks];
    __shared__ u64 slot_gain[kSelWaves], slot_tie[kSelWaves];
    __shared__ int32_t slot_t[kSelWaves];
    // M = 3: the (s0, s1) staircase of every prefix of P, descending s0 (and so
    // ascending s1); prefix j's corners from j (j + 1) / 2 on
    __shared__ uint2 stair[M == 3 ? 2 : 1][M == 3 ? kStair : 1];
    __shared__ int32_t stair_n[2][kHvMaxPicks];

    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t a = hdr[0], L = hdr[1] - a;
    const int32_t q = min(min(hdr[2], kHvMaxPicks), L - 1);   // (the level reaches past n_select: hdr[2] < L)
    const uint32_t nf = (uint32_t)hdr[3];
    const int32_t* lvl_do = lvl + n;
    constexpr int S = M == 2 ? 0 : 2;                  // the axis P is sorted along
    if (tid < kHvMaxPicks && tid >= q) {
        pick[tid] = -1;
        gain[tid] = 0;
    }
    if (q <= 0) return;                                // (uniform: the keys stay)

    for (int32_t cnt = 0; cnt < q; ++cnt) {
        const int buf = cnt & 1;
        Cand best{0, 0, -1};
        for (int32_t t = tid; t < L; t += kSel) {
            if (flag[t]) continue;
            uint32_t c[M];
            u64 vol = 1;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                c[m] = nf - lvl_r[(size_t)m * n + t];
                vol *= c[m];
            }
            u64 cov = 0;
            if constexpr (M == 2) {
                for (int j = 0; j < cnt; ++j) {
                    const uint32_t w = min(c[0], ps[0][j]);
                    const uint32_t wn = j + 1 < cnt ? min(c[0], ps[0][j + 1]) : 0u;
                    cov += (u64)(w - wn) * (u64)min(c[1], ps[1][j]);
                }
            } else {
                for (int j = 0; j < cnt; ++j) {
                    const uint32_t d = min(c[2], ps[2][j]);
                    const uint32_t dn = j + 1 < cnt ? min(c[2], ps[2][j + 1]) : 0u;
                    if (d == dn) continue;             // (every row of P deeper than c but the last)
                    const uint2* st = &stair[buf][j * (j + 1) / 2];
                    const int m_j = stair_n[buf][j];
                    u64 area = 0;
                    for (int k = 0; k < m_j; ++k) {
                        const uint32_t w = min(c[0], st[k].x);
                        const uint32_t wn = k + 1 < m_j ? min(c[0], st[k + 1].x) : 0u;
                        area += (u64)(w - wn) * (u64)min(c[1], st[k].y);
                    }
                    cov += (u64)(d - dn) * area;
                }
            }
            Cand me;
            me.gain = vol - cov;
            me.tie = ((u64)(uint32_t)lvl_do[t] << 32) | (u64)(uint32_t)~(uint32_t)lvl[t];
            me.t = t;
            if (better(me, best)) best = me;
        }
        best = wave_best(best);
        if (lane == 0) {
            slot_gain[wave] = best.gain;
            slot_tie[wave] = best.tie;
            slot_t[wave] = best.t;
        }
        __syncthreads();
        if (wave == 0) {
            Cand w{0, 0, -1};
            if (lane < kSelWaves) {
                w.gain = slot_gain[lane];
                w.tie = slot_tie[lane];
                w.t = slot_t[lane];
            }
            w = wave_best(w);
            // (q < L: an unpicked row exists, so w.t >= 0)
            uint32_t s[M];
#pragma unroll
            for (int m = 0; m < M; ++m) s[m] = nf - lvl_r[(size_t)m * n + w.t];
            if (lane == 0) {
                const int32_t row = lvl[w.t];
                pick[cnt] = row;
                gain[cnt] = w.gain;
                pick_t[cnt] = w.t;
                pick_i[cnt] = row;
                flag[w.t] = 1;
            }
            // the sorted insert: behind the rows that are not smaller along S
            uint32_t mine[M];
#pragma unroll
            for (int m = 0; m < M; ++m) mine[m] = lane < cnt ? ps[m][lane] : 0u;
            const int pos = __popcll(__ballot(lane < cnt && mine[S] >= s[S]));
            if (lane < cnt && lane >= pos) {
#pragma unroll
                for (int m = 0; m < M; ++m) ps[m][lane + 1] = mine[m];
            }
            if (lane == 0) {
#pragma unroll
                for (int m = 0; m < M; ++m) ps[m][pos] = s[m];
            }
            if constexpr (M == 3) if (lane <= cnt) {
                // the new prefix `lane`: before pos the old one, from pos on the
                // old prefix lane - 1 and the pick's (s0, s1)
                const int nb = buf ^ 1, j = lane;
                uint2* out = &stair[nb][j * (j + 1) / 2];
                int m_out = 0;
                if (j < pos) {
                    const uint2* in = &stair[buf][j * (j + 1) / 2];
                    m_out = stair_n[buf][j];
                    for (int k = 0; k < m_out; ++k) out[k] = in[k];
                } else {
                    const uint2* in = &stair[buf][j > 0 ? (j - 1) * j / 2 : 0];
                    const int m_in = j > 0 ? stair_n[buf][j - 1] : 0;
                    bool covered = false;
                    for (int k = 0; k < m_in; ++k) covered |= in[k].x >= s[0] && in[k].y >= s[1];
                    bool placed = covered;
                    for (int k = 0; k < m_in; ++k) {
                        const uint2 e = in[k];
                        if (!placed && e.x <= s[0]) {
                            out[m_out++] = make_uint2(s[0], s[1]);
                            placed = true;
                        }
                        if (covered || e.x > s[0] || e.y > s[1]) out[m_out++] = e;   // (else the pick covers it)
                    }
                    if (!placed) out[m_out++] = make_uint2(s[0], s[1]);
                }
                stair_n[nb][j] = m_out;
            }
        }
        __syncthreads();
    }

    // the level's keys: the picks from a in pick order, the others behind them
    if (tid < q) keys[pick_i[tid]] = (double)(a + tid);
    for (int32_t t = tid; t < L; t += kSel) {
        if (flag[t]) continue;
        int32_t before = 0;
        for (int k = 0; k < q; ++k) before += pick_t[k] < t ? 1 : 0;
        keys[lvl[t]] = (double)(a + q + t - before);
    }
}

}  // namespace

void hv_launch_prep(hipStream_t st, double* F, int32_t n, int32_t n_obj) {
    hipLaunchKernelGGL(k_hv_prep, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, F, n, n_obj);
}

void hv_launch_pairs(int32_t n_obj, dim3 grid, hipStream_t st, const double* F, int32_t n, int32_t per_slice,
                     int32_t* by, int32_t* dom, uint32_t* rank) {
    if (n_obj == 2)
        hipLaunchKernelGGL(k_hv_pairs<2>, grid, dim3(kBlock), 0, st, F, n, per_slice, by, dom, rank);
    else
        hipLaunchKernelGGL(k_hv_pairs<3>, grid, dim3(kBlock), 0, st, F, n, per_slice, by, dom, rank);
}

void hv_launch_select(int32_t n_obj, hipStream_t st, const uint64_t* sorted, int32_t n, int32_t bits,
                      const double* v, int32_t n_select, const uint32_t* rank, int32_t* hdr, int32_t* lvl,
                      uint32_t* lvl_r, unsigned char* flag, double* keys, int32_t* pick, u64* gain) {
    const dim3 rows((unsigned)((n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_hv_find, rows, dim3(kBlock), 0, st, sorted, n, bits, v, n_select, hdr);
    if (n_obj == 2) {
        hipLaunchKernelGGL(k_hv_compact<2>, rows, dim3(kBlock), 0, st, sorted, n, bits, rank, hdr, lvl, lvl_r, flag);
        hipLaunchKernelGGL(k_hv_select<2>, dim3(1), dim3(kSel), 0, st, hdr, lvl, lvl_r, flag, n, keys, pick, gain);
    } else {
        hipLaunchKernelGGL(k_hv_compact<3>, rows, dim3(kBlock), 0, st, sorted, n, bits, rank, hdr, lvl, lvl_r, flag);
        hipLaunchKernelGGL(k_hv_select<3>, dim3(1), dim3(kSel), 0, st, hdr, lvl, lvl_r, flag, n, keys, pick, gain);
    }
}

}  // namespace tpe_rt
