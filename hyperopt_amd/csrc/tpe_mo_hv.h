// tpe_mo_hv.h -- the launchers of tpe_mo_hv.hip (the hypervolume tie-break of
// the below set) for tpe_mo.hip's tpe_mo_keys_hv.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tpe_rt {

constexpr int kHvMaxPicks = 64;   // rows of the picked set the selection kernel keeps in LDS
constexpr int kHvHdr = 4;         // int32: level start a, level end, picks q, rank rows n_f

// The rows of F [n][n_obj] with a NaN set to NaN throughout, in place (the
// unconstrained call; k_moc_prep does it for the constrained one).
void hv_launch_prep(hipStream_t st, double* F, int32_t n, int32_t n_obj);

// k_mo_pairs<M> (tpe_mo.hip) that also counts, per objective, the rows j with
// F[j][m] < F[i][m]: rank[m][i], uint32[n_obj][n], zeroed by the caller.  n_obj 2 or 3.
void hv_launch_pairs(int32_t n_obj, dim3 grid, hipStream_t st, const double* F, int32_t n, int32_t per_slice,
                     int32_t* by, int32_t* dom, uint32_t* rank);

// From the sorted keys (by, n - do, i in `bits` bits each; v: the violations
// of the constrained call, or null): the level that straddles position
// n_select (0 < n_select < n), compacted, then the greedy picks and the keys
// of the level's rows.  hdr int32[kHvHdr]; lvl int32[2][n] (row, do); lvl_r
// uint32[n_obj][n]; flag [n]; pick int32[kHvMaxPicks]; gain uint64[kHvMaxPicks].
void hv_launch_select(int32_t n_obj, hipStream_t st, const uint64_t* sorted, int32_t n, int32_t bits,
                      const double* v, int32_t n_select, const uint32_t* rank, int32_t* hdr, int32_t* lvl,
                      uint32_t* lvl_r, unsigned char* flag, double* keys, int32_t* pick,
                      unsigned long long* gain);

}  // namespace tpe_rt
