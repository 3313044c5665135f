// Interpolated chroma, what yuv_linear.hip and the linear kernels of yuv_packed.hip share: the two taps
// of an axis with their weights in quarters, the horizontal sums of a run of chroma samples with its two halo samples, and
// the one rounding of the 2-D sum.  The result takes the place of the replicated sample in chroma() of yuv_samples.h, so the
// bytes are those of the replicate kernels on 4:4:4 planes holding the interpolated samples.
#pragma once
#include "yuv_samples.h"

namespace {

// an axis sub-sampled by 2, position p, k = p >> 1:  even p takes ea * C[k] + eb * C[k - 1],  odd p takes oa * C[k] + ob * C[k + 1]
// (indices clamped by the caller); each pair sums to 4.  An axis that is not sub-sampled has weight 4 on its own sample.
struct axis_taps { int ea, eb, oa, ob; };

__device__ __forceinline__ axis_taps axis_taps_of(int centred, int sub) {
    if (!sub) return {4, 0, 4, 0};
    if (centred) return {3, 1, 3, 1};       // sample k sits midway between positions 2k and 2k + 1
    return {4, 0, 2, 2};                    // sample k sits on position 2k
}

// s[0] the sample left of the run (clamped), s[1 .. NC] the run, s[NC + 1] the sample right of it (clamped) -> the 2 NC
// horizontal sums of the run's pixels, in quarters
template <int NC>
__device__ __forceinline__ void horizontal_sums(const int (&s)[NC + 2], const axis_taps& w, int (&h)[2 * NC]) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        h[2 * k] = w.ea * s[k + 1] + w.eb * s[k];
        h[2 * k + 1] = w.oa * s[k + 1] + w.ob * s[k + 2];
    }
}

// the interpolated sample: the pixel's own chroma row with weight wa, the other row with weight wb (wa + wb = 4), both as
// horizontal sums in quarters: sixteenths, rounded once
__device__ __forceinline__ int interpolated(int wa, int own, int wb, int other) { return (wa * own + wb * other + 8) >> 4; }

inline bool chroma_site_ok(const tdc_chroma_site* s) {
    return s && (s->sit_x == 0 || s->sit_x == 1) && (s->sit_y == 0 || s->sit_y == 1);
}

}  // namespace
