// tpe_mo_hvm.h -- the launcher of tpe_mo_hvm.hip (the sampled hypervolume
// indicator of raw rows against a reference point, two to eight objectives)
// for tpe_mo.hip's tpe_mo_exclusive_mc.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tpe_rt {

constexpr int kHvmMaxObj = 8;
constexpr int kHvmRow = 8;        // uint32 words of a row of thresholds: 32 bytes, one wave-uniform load
constexpr int kHvmStep = 4;       // rows k_hvm_cover tests between two looks at its exit condition
constexpr int kHvmTail = 2;       // uint32 behind count[n]: the covered samples, the alive rows

struct HvmRef {
    double r[kHvmMaxObj];
};

// The buffers of one call, all on the device.  n rows, M objectives, S samples.
struct HvmBufs {
    const double* F;          // [n][M] the rows (those k_moc_prep took out already NaN)
    double* lo;               // [kHvmMaxObj] the valid rows' minimum per axis
    uint32_t* T;              // [n + kHvmStep][kHvmRow] the thresholds, row-major, words M .. 7 zero
    unsigned char* alive;     // [n + kHvmStep] 1: valid and not thin; read four rows a word
    uint64_t* samp;           // [S] mode 0: uint32 first[S] in its front half; mode 1: (covers, clamped
                              //     to 2 a slice) << 32 | the sum of the slices' sole covering rows
    uint32_t* count;          // [n + kHvmTail]
};

// The row slices of k_hvm_cover's grid for n rows and S samples: enough
// workgroups for the chip when the samples alone are few, no slice shorter
// than 64 rows, every slice but the last a multiple of kHvmStep rows.  S = 64:
// a slice per 64 rows (n = 130: 44, 44, 42).
inline int32_t hvm_slices(int32_t n, int32_t S) {
    const int32_t blocks = (S + 255) / 256, want = 1024 / blocks;
    const int32_t most = (n + 63) / 64;
    return want < 1 ? 1 : (want < most ? want : most);
}

// count[i] (mode 0: the samples whose first covering alive row is i; 1: those
// that i alone covers), count[n] = the covered samples, count[n + 1] = the alive
// rows.  n_obj 2 .. 8, S a multiple of 64.  Enqueues only; the first error of a
// memset is returned, a launch error is left to hipGetLastError.
hipError_t hvm_launch(int32_t n_obj, hipStream_t st, const HvmBufs& b, int32_t n, HvmRef ref, int32_t mode,
                      int32_t S);

}  // namespace tpe_rt
