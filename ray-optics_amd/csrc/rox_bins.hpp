// rox_bins.hpp -- device helpers shared by the units that histogram rays (spotstats.hip, ee.hip,
// gmtf.hip, footprint.hip, wmaps.hip): the bin decision of numpy.histogram with explicit edges and
// with uniform ones, the wave-merged integer count and the wave-merged 64-bit integer sum.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rox {

// bin of v among edges e[0..n] as numpy.histogram with explicit edges decides it:
// searchsorted(e, v, 'right') - 1, the right-most edge belonging to the last bin; -1 = outside
__device__ __forceinline__ int bin_of(const double *e, int n, double v)
{
    if (!(v >= e[0]) || !(v <= e[n]))
        return -1;                              // (NaN included)
    int lo = 0, hi = n;                         // invariant: e[lo] <= v, (hi == n or v < e[hi])
    // uniform edges (linspace): the proportional guess is right or one off -- two probes
    const double w = e[n] - e[0];
    const double t = w > 0.0 ? (v - e[0]) / w * n : 0.0;
    int g = t < (double)(n - 1) ? (int)t : n - 1;
    if (e[g] <= v) {
        lo = g;
        if (g + 1 <= n && (g + 1 == n || v < e[g + 1]))
            return g;
    } else {
        hi = g;
    }
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// The bin of v among the n + 1 uniform edges lo + j * step (the last one hi) as numpy.histogramdd
// places it: searchsorted(edges, v, 'right') - 1, the last edge in the last bin; -1 = outside.
// The proportional guess is corrected by comparison with the edges themselves.  A box centred on
// 0 is (lo, hi) = (-h, h): v - (-h) is v + h, h - (-h) is h + h and -h + g * step is one IEEE
// operation either way, so the bin is the one the expressions written in h give, bit for bit.
__device__ __forceinline__ int uniform_bin(double v, double lo, double hi, double step, int n)
{
    if (!(v >= lo) || !(v <= hi))
        return -1;                              // (NaN included)
    const double t = (v - lo) / (hi - lo) * (double)n;
    int g = t < (double)(n - 1) ? (int)t : n - 1;
    g = g < 0 ? 0 : g;
    while (g > 0 && v < lo + (double)g * step)
        --g;
    while (g < n - 1 && v >= lo + (double)(g + 1) * step)
        ++g;
    return g;
}

// adds 1 per lane to h[b] for every lane with b >= 0: lanes of the same bin merge first --
// neighbouring rays of a grid land in the same bins (un-merged, a launch's atomics queue on few
// addresses: footprint.hip's maps took 20 x longer).  Every lane of the wave must call it.
__device__ __forceinline__ void wave_count(uint32_t *h, int b)
{
    const int lane = threadIdx.x & 63;
    uint64_t todo = __ballot(b >= 0);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int bl = __shfl(b, lead);
        const uint64_t same = __ballot(b == bl) & todo;
        if (lane == lead)
            atomicAdd(&h[bl], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// the weighted variant (wmaps.hip): adds q per lane to h[b], and 1 per lane to c[b] where c is
// given, for every lane with b >= 0.  Lanes of the same bin merge first: the leader adds their
// sum, gathered lane by lane where they are few and by a butterfly over the wave where they are
// many.  Integer sums: the result does not depend on which lanes merge.  Every lane of the wave
// must call it.
__device__ __forceinline__ void wave_add(unsigned long long *h, uint32_t *c, int b, unsigned long long q)
{
    const int lane = threadIdx.x & 63;
    uint64_t todo = __ballot(b >= 0);
    while (todo) {
        const int lead = __builtin_ctzll(todo);
        const int bl = __shfl(b, lead);
        const uint64_t same = __ballot(b == bl) & todo;
        const int n = __popcll(same);
        unsigned long long sum;
        if (n == 1) {
            sum = q;                            // (the leader's own: only the leader uses it)
        } else if (n <= 6) {
            sum = 0;
            for (uint64_t left = same; left; left &= left - 1)
                sum += __shfl(q, __builtin_ctzll(left));
        } else {
            sum = ((same >> lane) & 1) ? q : 0ull;
            for (int o = 32; o > 0; o >>= 1)
                sum += __shfl_xor(sum, o);
        }
        if (lane == lead) {
            atomicAdd(&h[bl], sum);
            if (c)
                atomicAdd(&c[bl], (uint32_t)n);
        }
        todo &= ~same;
    }
}

}  // namespace rox
