// tpe_mo_hvx4.h -- the launcher of tpe_mo_hvx4.hip (exclusive hypervolumes of
// raw four-objective rows against a reference point) for tpe_mo.hip's
// tpe_mo_exclusive4.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tpe_rt {

constexpr int kHvx4Cap = 512;   // clipped rows a live row's workgroup keeps in LDS (TPE_OPT_MO_HVX_CAP lowers it)
constexpr int kHvx4Hdr = 2;     // int32: live rows, live rows whose kept set outgrew the capacity

struct Hvx4Ref {
    double r[4];
};

// F [n][4] (the rows k_moc_prep took out already NaN), in place: every row that
// is not finite or not below ref on every axis set to NaN; then excl[i] for
// every row -- 0 for a row that is not valid or that a row of its J (mode 0: the
// valid rows before it, 1: every other valid row) weakly dominates, NaN (counted
// in hdr[1]) when its kept set outgrew cap, its exclusive hypervolume otherwise.
// pair_grid, per_slice: k_mo_pairs' split of the pairs.  flag int32[n], live
// int32[n], hdr int32[kHvx4Hdr], excl double[n].
void hvx4_launch(hipStream_t st, double* F, int32_t n, Hvx4Ref ref, int32_t mode, int32_t cap, dim3 pair_grid,
                 int32_t per_slice, int32_t* flag, int32_t* live, int32_t* hdr, double* excl);

}  // namespace tpe_rt
