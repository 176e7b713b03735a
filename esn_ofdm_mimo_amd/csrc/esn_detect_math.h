// The arithmetic of the detector tail for every kernel that computes X = FFT_N(y) / (N sqrt(Pi)) and
// slices it: esn_detect.hip (the generic kernel and the fixed-shape instances) and esn_remod.hip (decide and
// re-modulate).  They compile the same operations on the same operands (the library is built with -ffp-contract=off:
// every product and sum below is rounded on its own), so their spectra, indices and counters are bit-identical.  The
// multiplications by the twiddles (1, -0) and (0, -1) stay: dropping them flips signed zeros.
#pragma once
#include "esn_common.h"

namespace esn {

__device__ __forceinline__ void det_bfly(double2& a, double2& c, const double2 w) {
    const double tr = c.x * w.x - c.y * w.y, ti = c.x * w.y + c.y * w.x;
    const double2 a0 = a;
    a = make_double2(a0.x + tr, a0.y + ti);
    c = make_double2(a0.x - tr, a0.y - ti);
}
__device__ __forceinline__ double2 det_twiddle(int k, int N) {      // exp(-2 pi i k / N)
    double sn, cs;
    sincospi(-2.0 * (double)k / (double)N, &sn, &cs);
    return make_double2(cs, sn);
}
__device__ __forceinline__ double det_norm(int side) { return sqrt(2.0 * (double)(side * side - 1) / 3.0); }
__device__ __forceinline__ double det_scale(int N, double p_i_g) { return 1.0 / ((double)N * sqrt(p_i_g)); }
__device__ __forceinline__ int det_slice(double v, double norm, int side) {   // index of the nearest grid level
    const int i = (int)rint((v * norm + (double)(side - 1)) * 0.5);
    return min(max(i, 0), side - 1);
}

}  // namespace esn
