// rox_packets.hpp -- what the entries that walk the ROX_OUT_FULL packets of finished launches share
// (footprint.hip, fresnel.hip, solidangle.hip, segfoci.hip, wmaps.hip, wavediff.hip): their argument checks, a
// system's slot tables as their kernels read them, the tile their workgroups walk, the fixed-order
// merge of a wave's records and that of their finishing kernels, and the carried direction of
// fresnel.hip and wavediff.hip.
#pragma once

#include <cstring>
#include <type_traits>

#include "rox_host.hpp"

namespace rox {

constexpr int kRtDoubles = 10;                  // an interface's staged row: rt[9], rt_order

// ---- argument checks (as rox_host.hpp's); an entry calls them in its own order
inline int check_packet_call(const char *e, const rox_system *sys, const rox_out *outs, int32_t n_items)
{
    if (!sys || !outs)
        return host_fail(ROX_E_ARG, "%s: null sys or outs", e);
    return check_range(e, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS);
}

inline int check_packet_rays(const char *e, int64_t n_rays)
{
    if (n_rays < 1 || n_rays > (int64_t(1) << 28))
        return host_fail(ROX_E_ARG, "%s: n_rays %lld outside [1, 2^28]", e, (long long)n_rays);
    return 0;
}

// item i: the rows the entry reads are there and hold n_rays rays
inline int check_packet_item(const char *e, int32_t i, const rox_out &out, int64_t n_rays, bool need_fail_surf)
{
    if (!out.seg || !out.status || (need_fail_surf && !out.fail_surf))
        return host_fail(ROX_E_ARG, "%s: item %d: null %s", e, i,
                         need_fail_surf ? "seg, status or fail_surf" : "seg or status");
    if (out.ld < n_rays)
        return host_fail(ROX_E_ARG, "%s: item %d: ld %lld < n_rays %lld", e, i, (long long)out.ld, (long long)n_rays);
    return 0;
}

// ---- a system's interfaces and the FULL-packet slots of launches traced with trace_flags
struct PacketSlots {
    int32_t n_ifcs = 0, n_seg = 0;
    const rox_surface *rows;                    // system_rows
    std::vector<int32_t> slots;                 // system_slot_map

    PacketSlots(const rox_system *sys, uint32_t trace_flags) : rows(system_rows(sys, &n_ifcs))
    {
        system_slot_map(sys, (trace_flags & ROX_FILTER_PHANTOMS) != 0, slots, n_seg);
    }

    // dst[n_ifcs][kRtDoubles]: rt, then 1.0 for ROX_RT_C_ORDER and 0.0 for ROX_RT_F_ORDER
    void stage_rt(double *dst) const
    {
        for (int32_t i = 0; i < n_ifcs; ++i, dst += kRtDoubles) {
            memcpy(dst, rows[i].rt, sizeof(double) * 9);
            dst[9] = rows[i].rt_order == ROX_RT_C_ORDER ? 1.0 : 0.0;
        }
    }

    // dst[n_seg]: the interface of slot k
    void stage_slot_ifc(int32_t *dst) const
    {
        for (int32_t i = 0; i < n_ifcs; ++i)
            if (slots[i] >= 0)
                dst[slots[i]] = i;
    }
};

// ---- a ray's direction carried from one slot's frame into the next (rox_surface_transmission's
// statement of it, which rox_wave_differentials promises to follow): three doubles, the dot and
// cross products in the operation order include/roxtrace.h gives, and rt . v with the columns
// summed in the row's rt_order, unfused.  P is a pointer to the staged row (kRtDoubles).
struct V3 {
    double x, y, z;
};

__device__ __forceinline__ double dot(const V3 &a, const V3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(const V3 &a, const V3 &b)
{
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

template <class P>
__device__ __forceinline__ V3 carry(P rt, bool c_order, const V3 &v)
{
    if (c_order)
        return V3{(rt[1] * v.y + rt[0] * v.x) + rt[2] * v.z, (rt[4] * v.y + rt[3] * v.x) + rt[5] * v.z,
                  (rt[7] * v.y + rt[6] * v.x) + rt[8] * v.z};
    return V3{(rt[0] * v.x + rt[1] * v.y) + rt[2] * v.z, (rt[3] * v.x + rt[4] * v.y) + rt[5] * v.z,
              (rt[6] * v.x + rt[7] * v.y) + rt[8] * v.z};
}

// ---- the tile walk: a workgroup of kBlock threads owns kTile consecutive rays of one item
// (blockIdx.y), kRays per thread, ray j of a thread kBlock rays after its ray j - 1, so that a wave
// reads 64 consecutive rays; each of its kWaves waves writes one partial record per slot
template <int kRaysPerThread>
struct PacketTile {
    static constexpr int kBlock = 256;
    static constexpr int kWaves = kBlock / 64;
    static constexpr int kRays = kRaysPerThread;
    static constexpr int kTile = kBlock * kRays;

    // workgroups per item
    static int tiles(int64_t n_rays) { return (int)((n_rays + kTile - 1) / kTile); }
    // ray j of this thread, in a launch whose first ray is ray0
    static __device__ __forceinline__ int64_t ray(int j, int64_t ray0 = 0)
    {
        return ray0 + (int64_t)blockIdx.x * kTile + j * kBlock + threadIdx.x;
    }
    // this wave's first partial record in part[items][n_waves][n_seg], n_waves over all of an
    // item's rays (ray0 a multiple of kTile)
    static __device__ __forceinline__ size_t part(int n_waves, int n_seg, int64_t ray0 = 0)
    {
        return ((size_t)blockIdx.y * n_waves + (size_t)(ray0 / kTile + blockIdx.x) * kWaves + (threadIdx.x >> 6)) *
               n_seg;
    }
};

// ---- the merge of a wave: t becomes the 64 lanes' records merged by the fixed butterfly
// o = 32, 16, .., 1 of merge(t, partner), the lane's own record first (the callers write lane 0's).
// The record travels as 32-bit words, whatever its fields: one added to a record is merged with it.
template <class T>
__device__ __forceinline__ T shfl_xor(const T &a, int o)
{
    static_assert(std::is_trivially_copyable<T>::value, "a record is shuffled as its bytes");
    static_assert(sizeof(T) % 4 == 0, "a record is shuffled as 32-bit words");
    constexpr int n = (int)(sizeof(T) / 4);
    int w[n];
    __builtin_memcpy(w, &a, sizeof(T));
#pragma unroll
    for (int i = 0; i < n; ++i)
        w[i] = __shfl_xor(w[i], o);
    T b;
    __builtin_memcpy(&b, w, sizeof(T));
    return b;
}

template <class T, class Merge>
__device__ __forceinline__ void wave_merge(T &t, Merge merge)
{
    for (int o = 32; o > 0; o >>= 1) {
        const T b = shfl_xor(t, o);
        merge(t, b);
    }
}

// ---- the merge of a finishing kernel, by a workgroup of kBlock threads: the n records p[w * stride]
// into one, in one fixed order whatever the launch -- thread t merges w = t, t + kBlock, ... in that
// order into `init`, then the threads merge as a binary tree through lds[kBlock], the lower thread's
// first.  merge(a, b) is a <- a merged with b, for b a record and for b a merged value.
template <int kBlock, class In, class T, class Merge>
__device__ __forceinline__ T block_merge(const In *__restrict__ p, int n, int stride, T init, Merge merge, T *lds)
{
    const int t = threadIdx.x;
    for (int w = t; w < n; w += kBlock) {
        // a copy, here and of lds[t + h]: a record's loads are issued together, not one where each
        // value is first used (footprint_finish took 8 us longer per launch at 4096 waves without it)
        const In q = p[(size_t)w * stride];
        merge(init, q);
    }
    lds[t] = init;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (t < h) {
            T m = lds[t];
            const T o = lds[t + h];
            merge(m, o);
            lds[t] = m;
        }
        __syncthreads();
    }
    return lds[0];
}

}  // namespace rox
