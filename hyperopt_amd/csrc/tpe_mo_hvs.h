// tpe_mo_hvs.h -- the launchers of tpe_mo_hvs.hip (the sampled hypervolume
// tie-break of the below set, two to eight objectives) for tpe_mo.hip's
// tpe_mo_keys_hvs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tpe_rt {

constexpr int kHvsMaxObj = 8;
constexpr int kHvsMaxPicks = 64;
constexpr int kHvsHdr = 4;        // int32: level start a, level end, picks q, rank rows n_f

// The buffers of one call, all on the device.  n rows, M objectives, S samples,
// W = S / 64 words; L, the level's rows, is known to the host from `hdr` on.
struct HvsBufs {
    const uint64_t* sorted;   // [n] tpe_mo_keys' sorted keys (by, n - do, i in `bits` bits each)
    const double* v;          // [n] the violations of the constrained call, or null
    const uint32_t* rank;     // [M][n]
    int32_t* hdr;             // [kHvsHdr]
    int32_t* lvl;             // [2][n]  the level's rows, their do
    uint32_t* lvl_r;          // [M][n]  the level's ranks
    unsigned char* flag;      // [n]     picked
    uint32_t* lo;             // [kHvsMaxObj]
    uint32_t* pts;            // [M][S]  the samples, axis-major
    uint64_t* bits;           // [W][L]  bit s % 64 of bits[s / 64][c]: row c covers sample s
    uint64_t* covered;        // [W]     the samples P covers
    uint32_t* cgain;          // [L]     the gains of one pick (zero between picks)
    int32_t* pick;            // [kHvsMaxPicks] the picks' rows
    int32_t* pick_t;          // [kHvsMaxPicks] their places in the level
    unsigned long long* gain; // [kHvsMaxPicks]
    double* keys;             // [n]
};

// k_mo_pairs<M> (tpe_mo.hip) that also counts, per objective, the rows j with
// F[j][m] < F[i][m]: rank[m][i], uint32[n_obj][n], zeroed by the caller.  n_obj 2 .. 8.
void hvs_launch_pairs(int32_t n_obj, dim3 grid, hipStream_t st, const double* F, int32_t n, int32_t per_slice,
                      int32_t* by, int32_t* dom, uint32_t* rank);

// The level that straddles position n_select (0 < n_select < n) and its rows
// gathered to the front of lvl, lvl_r; flag cleared.  The host reads hdr next.
void hvs_launch_level(int32_t n_obj, hipStream_t st, const HvsBufs& b, int32_t n, int32_t bits, int32_t n_select);

// With hdr on the host (L rows from position a, q picks, n_f rank rows): the
// samples, the coverage matrix, q picks and the keys of the level's rows.
void hvs_launch_select(int32_t n_obj, hipStream_t st, const HvsBufs& b, int32_t n, int32_t a, int32_t L, int32_t q,
                       int32_t n_f, int32_t n_samples);

}  // namespace tpe_rt
