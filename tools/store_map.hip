// store_map.hip -- where do the FULL packet stores land?  Two store-only probes.
//  (a) "stride": kStreams workgroups each write one 4 KiB block per pass, the blocks of a pass
//      `stride` bytes apart, for stride = 4 KiB ... 64 MiB in powers of two and each of them
//      + 2 KiB and + 4 KiB.  Every block of a launch is a different one (2 GiB written, spread
//      over a window of kStreams x 64 MiB), so no cache absorbs the stream.  Where the rate
//      falls, the blocks of a pass share a channel (or a bank): the cliffs give the interleave
//      granule and the periods of the address map.
//  (b) "shape": the shipped store shape -- 1024 workgroups of 1024 threads, SoA rows
//      [segment][component][ray], a barrier per segment, ten 8-byte nt stores per lane and
//      segment in bursts of 4 / 3 / 3, optionally `work` dependent fp64 FMAs in front of each
//      burst (the trace arithmetic's place) -- with the row pitch (n + pad doubles) and the
//      workgroup -> tile map (rox_args.hpp full_tile_map(), `group` tiles per XCD run) as
//      parameters.
//   hipcc --offload-arch=gfx950 -O3 tools/store_map.hip -o store_map && ./store_map [stride|shape]
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int kStreams = 512;           // (a): workgroups = blocks written at once
constexpr int kBlockBytes = 4096;       // (a): 512 lanes x 8 B
constexpr int kPasses = 1024;           // (a): blocks per workgroup and launch (2 GiB a launch)

// pass i, workgroup k writes block i * kStreams + k at that index x stride, folded into the
// window; every fold moves on by one block so that a launch never writes an address twice
// (power-of-two strides; the others may graze an earlier block, which costs nothing)
// (the window is 2^window_log2 bytes: a division per pass would bound the probe, not the stores)
__global__ void __launch_bounds__(512) stride_blocks(char *buf, int window_log2, size_t alloc, size_t stride)
{
#pragma unroll 4
    for (int i = 0; i < kPasses; ++i) {
        const size_t lin = ((size_t)i * kStreams + blockIdx.x) * stride;
        const size_t at = (lin & (((size_t)1 << window_log2) - 1)) + (lin >> window_log2) * kBlockBytes;
        if (at + kBlockBytes > alloc)
            continue;
        __builtin_nontemporal_store((double)i, reinterpret_cast<double *>(buf + at) + threadIdx.x);
    }
}

// the tile map of the trace kernel (csrc/rox_args.hpp full_tile_map(), wg0 = 0)
__host__ __device__ constexpr long tile_map(long t, long n_tiles, int group)
{
    if (group <= 0)
        return t;
    const long span = 8L * group, start = t / span * span;
    if (start + span > n_tiles)
        return t;
    const long j = t - start;
    return start + j % 8 * group + j / 8;
}

__global__ void __launch_bounds__(1024) shape(double *out, long ld, long n_tiles, int segs, int group, int work)
{
    const long r = tile_map(blockIdx.x, n_tiles, group) * 1024 + threadIdx.x;
    double v = (double)r, w = 1.0 + 1e-9 * threadIdx.x;
    for (int sg = 0; sg < segs; ++sg) {
        __builtin_amdgcn_s_barrier();
        double *base = out + (long)sg * 10 * ld + r;
#pragma unroll
        for (int c0 = 0; c0 < 10; c0 += (c0 == 0 ? 4 : 3)) {        // bursts of 4 / 3 / 3
            for (int i = 0; i < work; ++i)
                w = fma(w, 1.0000001, 1e-12);
            v += w;
#pragma unroll
            for (int c = c0; c < c0 + (c0 == 0 ? 4 : 3); ++c)
                __builtin_nontemporal_store(v + c, base + (long)c * ld);
        }
    }
}

template <class F>
double time_us(F f, int warm, int reps)
{
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    for (int i = 0; i < warm; ++i) f();
    CHECK(hipEventRecord(a));
    for (int i = 0; i < reps; ++i) f();
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    CHECK(hipGetLastError());
    float ms; CHECK(hipEventElapsedTime(&ms, a, b));
    CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
    return ms * 1e3 / reps;
}

static void run_stride()
{
    // the window holds one pass at the largest stride; a smaller device gets a smaller sweep
    size_t max_stride = (size_t)64 << 20;
    char *buf = nullptr;
    size_t window = 0, alloc = 0;
    for (; max_stride >= ((size_t)1 << 20); max_stride >>= 1) {
        window = kStreams * max_stride;
        alloc = window + max_stride + (1 << 16);
        if (hipMalloc(&buf, alloc) == hipSuccess)
            break;
        (void)hipGetLastError();
        buf = nullptr;
    }
    if (!buf) { printf("{\"probe\": \"stride\", \"error\": \"no window\"}\n"); return; }
    int window_log2 = 0;
    while (((size_t)1 << window_log2) < window)
        ++window_log2;
    const double bytes = (double)kStreams * kPasses * kBlockBytes;
    for (size_t s = 4096; s <= max_stride; s <<= 1)
        for (size_t extra : {(size_t)0, (size_t)2048, (size_t)4096}) {
            const size_t stride = s + extra;
            const double t = time_us([&] { hipLaunchKernelGGL(stride_blocks, dim3(kStreams), dim3(512), 0, 0,
                                                              buf, window_log2, alloc, stride); }, 2, 5);
            printf("{\"probe\": \"stride\", \"stride\": %zu, \"pow2\": %zu, \"plus\": %zu, \"us\": %.1f, \"GBps\": %.0f}\n",
                   stride, s, extra, t, bytes / t / 1e3);
            fflush(stdout);
        }
    CHECK(hipFree(buf));
}

static void run_shape()
{
    const long n = 1024L * 1024, n_tiles = n / 1024;
    const int segs = 12;
    const long pads[] = {0, 32, 64, 128, 256, 512, 768, 1024, 1280, 2304, 4352, 8448, 16640, 33024, 65280, 65536};
    const long max_pad = 65536;
    double *buf;
    CHECK(hipMalloc(&buf, (size_t)segs * 10 * (n + max_pad) * 8));
    const double bytes = (double)segs * 10 * n * 8;
    for (int work : {0, 25})
        for (int round = 0; round < 2; ++round)
            for (long pad : pads)
                for (int group : {0, 1, 2, 4, 8, 16, 32, 64, 128}) {
                    const long ld = n + pad;
                    const double t = time_us([&] { hipLaunchKernelGGL(shape, dim3((unsigned)n_tiles), dim3(1024), 0, 0,
                                                                      buf, ld, n_tiles, segs, group, work); }, 10, 40);
                    printf("{\"probe\": \"shape\", \"work\": %d, \"round\": %d, \"pad\": %ld, \"group\": %d, \"us\": %.1f, \"GBps\": %.0f}\n",
                           work, round, pad, group, t, bytes / t / 1e3);
                    fflush(stdout);
                }
    CHECK(hipFree(buf));
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "all";
    if (!strcmp(what, "stride") || !strcmp(what, "all"))
        run_stride();
    if (!strcmp(what, "shape") || !strcmp(what, "all"))
        run_shape();
    return 0;
}
