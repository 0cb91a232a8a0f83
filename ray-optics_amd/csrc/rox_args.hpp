// rox_args.hpp -- what the host units and the kernels share: the device row of the surface table,
// the kernel argument blocks, the launch configuration, the tables of instance entry points and
// the tile geometry both sides compute.  Nothing here is __device__-only: the host units
// (launch.hip, the entry units) include this and no kernel code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rox_config.hpp"

namespace rox {

static_assert(sizeof(rox_aperture) == 40, "rox_aperture layout");
static_assert(sizeof(rox_phase) == 168, "rox_phase layout");
static_assert(sizeof(rox_surface) == 576, "rox_surface layout");
static_assert(sizeof(rox_field) == 192, "rox_field layout");
static_assert(sizeof(rox_enp) == 136, "rox_enp layout");
static_assert(sizeof(rox_pupil_iter) == 224, "rox_pupil_iter layout");

// Device-side row = the public rox_surface + per-surface values that are the
// same for every ray and are therefore computed once at rox_system_create:
// dcoefs[i] = c_coef_i * coefs[i], the product the df() loops of the polynomial
// profiles form per evaluation (c_coef_i = 2(i+1), or i+1 for RadialPolynomial;
// exact small integers, so the host product has the reference's rounding).
// cd[] interleaves (coefs[i], dcoefs[i]): the sag and slope series read one
// 16-byte LDS word per term.
struct dev_surface {
    rox_surface pub;
    double cd[2 * ROX_MAX_COEF];
};
constexpr int kRowDoubles = sizeof(dev_surface) / sizeof(double);   // 92
static_assert(offsetof(dev_surface, cd) % 16 == 0 && sizeof(dev_surface) % 16 == 0, "16-byte LDS reads");
// Per (wavelength, interface) constants of a DiffractionGrating, formed on the
// host with libm pow() exactly as the reference's `mu**2` / `T**2` are:
//   [0] mu = n_in/n_out  [1] mu**2  [2] T  [3] T**2          (doe.py:138-143)
constexpr int kPhaseConsts = 4;

// ---------------------------------------------------------------- kernel args
struct TraceArgs {
    const double *rows;        // [N][kRowDoubles] dev_surface rows
    const double *n_table;     // [W][N]
    const double *ph_consts;   // [W][N][kPhaseConsts] or nullptr
    const double *wvls;        // [W] nm
    const int32_t *slots;      // [2][N]: slot[s] (-1 = filtered phantom), nslots_before[s]
    int32_t n_ifcs, n_wvls;
    int64_t n_rays;            // rays of this launch (<= 2^28: 32-bit lane byte offsets)
    int64_t ray_base;          // index of this launch's first ray within the batch
    int64_t in_ld;             // batch size = stride of the SoA inputs
    // explicit rays
    const double *pt0, *dir0;  // SoA [3][n_rays]
    const int32_t *wvl_idx;    // per ray or nullptr
    int32_t wvl_idx_all;
    // pupil rays
    const double *px, *py;     // axis / list coordinates
    int32_t axis_kind;         // AXIS_LIST: px[r],py[r]; AXIS_PRODUCT: px[r/num], py[r%num]
    int32_t axis_num;
    int32_t row_begin;         // AXIS_PRODUCT: first pupil row of this launch
    // HITS_COMPACT: decoupled look-back state of this launch
    uint64_t *tile_state;      // [tiles] (epoch << 32 | flag << 30 | count)
    uint32_t *ticket;          // [0] next tile, [1] workgroups done
    // pairs already in out.seg when this launch starts (earlier launches of a chunked
    // call; earlier calls with ROX_HITS_APPEND) -- nullptr = none -- and where the running
    // total goes.  Never the same word: a tile may still be reading the base while the
    // last tile already knows the total (the host ping-pongs two slots between launches).
    const int64_t *hits_base_in;
    int64_t *hits_total_out;
    uint32_t epoch;
    // the first `small_tiles` tickets are tiles of kSmallTile rays (see compact_tiles())
    int32_t small_tiles;
    // FULL: tiles per XCD run of the workgroup -> tile map (full_tile_map()); 0 = identity
    int32_t tile_group;
    rox_field fld;
    rox_opts opts;
    rox_out out;
};

// the through-focus launch (MODE_FOCUS): a pupil-grid launch plus its focus planes and outputs
struct FocusArgs : TraceArgs {
    const rox_focus_plane *planes;  // [n_planes], device memory, read through scalar loads
    int32_t n_planes;
    double *focus_rows;             // [n_planes][3][out.ld] or nullptr
    double *partial;                // FocusAcc [gridDim.x][waves per workgroup][n_planes] or nullptr
};

// A batch of up to kInlineItems items travels IN the kernel argument (`inl`, `items` null): no
// upload in front of the kernel -- a copy-engine transfer and its cross-queue signal, ~6 us
// before an 18-30 us kernel of a figure's or BASELINE configs[3]'s few small grids.  (gfx950
// takes kernel arguments of 31 KiB and more; tools/kernarg_probe.hip: a launch with 16 items
// inline 4.6 us against 7.0 us for upload + launch, back to back.)
constexpr int kInlineItems = 16;
struct BatchArgs {
    const TraceArgs *items;             // device array [gridDim.y], or nullptr: the items are inl[]
    TraceArgs inl[kInlineItems];
};

// HITS_COMPACT tile geometry.  The first `want` tickets of a launch take tiles of kSmallTile
// rays: a 1024-thread workgroup then runs four waves, one per SIMD, and is through its
// surfaces in a third of the time sixteen take.  The host asks for them when the whole launch
// fits one small tile per CU (a 256 x 256 grid spreads over 256 CUs instead of 64); later
// tickets take full tiles.
constexpr int kSmallTile = 256;
__host__ __device__ inline int64_t compact_small_tiles(int64_t n_rays, int32_t want)
{
    const int64_t fit = n_rays / kSmallTile;
    return want < fit ? (want < 0 ? 0 : want) : fit;
}
__host__ __device__ inline int64_t compact_tiles(int64_t n_rays, int32_t want_small, int kB)
{
    const int64_t s = compact_small_tiles(n_rays, want_small);
    return s + (n_rays - s * kSmallTile + kB - 1) / kB;
}

// FULL tile placement.  The hardware deals consecutive workgroups of a launch round-robin over
// the kXcds dies, so under the identity map die x writes tiles x, x + 8, ...: consecutive row
// pieces of a packet row leave through eight different L2s.  full_tile_map() permutes the walk
// index t of trace_tiles() (workgroup + pass x grid) so that, over each whole block of
// kXcds * group consecutive tiles, the walk indices of one die -- those with (t + wg0) % kXcds
// equal, wg0 the linear id of the item's first workgroup -- get `group` contiguous tiles.  The
// ragged remainder and group <= 0 keep the identity.  A bijection of [0, n_tiles) for every
// wg0 and grid; the die it names is the workgroup's own wherever the grid is a multiple of
// kXcds (every capped grid on a chip whose CU count is).
constexpr int kXcds = 8;
// (32-bit arithmetic: a launch has at most 2^28 rays, so fewer than 2^31 tiles; group is
// clamped by the host to kMaxTileGroup)
constexpr int32_t kMaxTileGroup = 1 << 16;
__host__ __device__ constexpr int64_t full_tile_map(int64_t t, int64_t n_tiles, int32_t group, uint32_t wg0)
{
    if (group <= 0)
        return t;
    const uint32_t span = (uint32_t)kXcds * (uint32_t)group;
    const uint32_t start = (uint32_t)t / span * span;
    if ((int64_t)start + span > n_tiles)
        return t;
    const uint32_t j = (uint32_t)t - start;
    return (int64_t)(start + (j + wg0) % kXcds * (uint32_t)group + j / kXcds);
}

// ------------------------------------------------------------------ through focus
// Statistics: a wave forms its own (count, means, sums of squared deviations from its means) in
// two passes over its lanes (butterfly sums), and one lane merges that into the wave's partial
// record of the plane (Chan, Golub & LeVeque's pairwise update): an OPD of -472 waves that
// varies by 0.02 keeps its RMS, which sum(w^2)/n - mean^2 loses in cancellation.  No atomics, a
// fixed order of merges -- the finishing pass (focus.hip) merges the records in index order
// -- so two identical calls give bit-identical statistics.
struct FocusAcc {
    double n;               // rays with status OK
    double mx, my;          // centroid
    double m2xy;            // sum of (x - mx)^2 + (y - my)^2
    double sr2;             // sum of x^2 + y^2 (about image_pt)
    double mw, m2w;         // OPD mean and sum of (w - mw)^2
    double wmin, wmax;      // (records start zeroed, n = 0: focus_merge never reads them then)
};
constexpr int kFocusStat = sizeof(FocusAcc) / sizeof(double);

__host__ __device__ inline FocusAcc focus_merge(const FocusAcc &a, const FocusAcc &b)
{
    if (b.n == 0)
        return a;
    if (a.n == 0)
        return b;
    FocusAcc r;
    r.n = a.n + b.n;
    const double f = b.n / r.n, g = a.n * b.n / r.n;
    const double dx = b.mx - a.mx, dy = b.my - a.my, dw = b.mw - a.mw;
    r.mx = a.mx + dx * f;
    r.my = a.my + dy * f;
    r.m2xy = (a.m2xy + b.m2xy) + (dx * dx + dy * dy) * g;
    r.sr2 = a.sr2 + b.sr2;
    r.mw = a.mw + dw * f;
    r.m2w = (a.m2w + b.m2w) + dw * dw * g;
    r.wmin = fmin(a.wmin, b.wmin);
    r.wmax = fmax(a.wmax, b.wmax);
    return r;
}

// ------------------------------------------------------------------ launching
struct LaunchCfg {
    int gen;            // GEN_*
    bool per_ray_wvl;
    bool small;         // workgroups of ROX_BLOCK_SMALL threads (pupil launches; see block_of())
    bool fast;          // the tolerance-mode instance (ROX_FAST_FP64 on a reduced-output mode)
    bool gtab;          // the table does not fit the LDS: the general instance over global memory
    int n_inline;       // batches: > 0 = `items` is a HOST array of this many items for the kernel argument
    int out_mode;       // ROX_OUT_*
    dim3 grid;
    size_t lds;
    hipStream_t stream;
};

// The host entry points of one trace instance: the plain, batched and through-focus launches of
// launch_instance*<FEAT>.  ROX_TRACE_INSTANCE defines them as one table entry trace_<name>
// in the instance's own translation unit.  (The entries are not const: clang would emit a const
// namespace-scope object into the device code object as well.)
struct TraceInstanceFns {
    void (*launch)(const LaunchCfg &, const TraceArgs &);
    void (*batch)(const LaunchCfg &, const TraceArgs *);
    void (*focus)(const LaunchCfg &, const FocusArgs *);
};
#define ROX_TRACE_DECL(name, FEAT) extern TraceInstanceFns trace_##name, trace_##name##_fast;
ROX_TRACE_INSTANCES(ROX_TRACE_DECL)
extern TraceInstanceFns trace_general_gtab;
#undef ROX_TRACE_DECL

// the pack pass of two-pass packed hits (csrc/pack.hip): a plain ROX_OUT_HITS launch has left
// (x, y)[2][ld] and status[n_rays]; survivors go to dst in ray order, exactly where the fused
// HITS_COMPACT instance would have put them (same tile-state / ticket / base / total protocol)
struct PackArgs {
    const uint8_t *status;
    const double *xy;          // [2][ld]
    int64_t ld, n_rays;
    uint64_t *tile_state;
    uint32_t *ticket;          // [0] next tile, [1] workgroups done
    const int64_t *hits_base_in;
    int64_t *hits_total_out;
    uint32_t epoch;
    double *dst;               // rox_out.seg of the HITS_COMPACT call: (x, y) pairs
    int64_t ld_dst;            // its capacity in pairs (rox_out.ld)
};
constexpr int kPackBlock = 1024, kPackSub = 4, kPackTile = kPackBlock * kPackSub;
void launch_pack(const PackArgs &, unsigned blocks, hipStream_t);

// chief-ray aiming (csrc/rox_search.hpp)
struct AimArgs {
    const double *rows, *n_table, *ph_consts, *wvls;
    const int32_t *slots;
    int32_t n_ifcs, n_wvls, n;
    const rox_aim *probs;      // device
    double eps;
    double *aim_xy;            // device [n][2]
    int32_t *result;           // device [n]
    double *last_xy;           // device [n][2] or nullptr: the last trial ray's (x1, y1)
    int32_t *last_status;      // device [n] or nullptr: ... and its trace status
    int32_t wave_per_problem;  // 1: one wave (block) per problem; 0: one lane per problem
};

// wide-angle pupil search (csrc/rox_search.hpp)
struct EnpArgs {
    const double *rows, *n_table, *ph_consts, *wvls;
    const int32_t *slots;
    int32_t n_ifcs, n_wvls, n;
    const rox_enp *probs;      // device
    double eps;
    double *z_out;             // device [n][2]
    int32_t *result;           // device [n]
};

// vignetting search (csrc/rox_search.hpp)
struct VigArgs {
    const double *rows, *n_table, *ph_consts, *wvls;
    const int32_t *slots;
    int32_t n_ifcs, n_wvls, n;
    const rox_vig *probs;      // device
    double eps;
    double *vig;               // device [n]
    int32_t *clip;             // device [n]
    // rox_iterate_pupil_rays: iterate_pupil_ray on its own (probs unused, vig = start_r)
    const rox_pupil_iter *iters;
    int32_t wave_per_problem;  // 1: one wave (block) per problem; 0: one lane per problem
};

// The host entry points of one search instance (rox_search.hpp launch_*_instance<FEAT>), defined
// as one table entry search_<name> by ROX_SEARCH_INSTANCE in csrc/search_<name>.hip (not const,
// as TraceInstanceFns)
struct SearchInstanceFns {
    void (*aim)(const AimArgs &, size_t lds, hipStream_t);
    void (*enp)(const EnpArgs &, size_t lds, hipStream_t);
    void (*vig)(const VigArgs &, size_t lds, hipStream_t);
};

#define ROX_SEARCH_DECL(name, FEAT) extern SearchInstanceFns search_##name;
ROX_SEARCH_INSTANCES(ROX_SEARCH_DECL)
extern SearchInstanceFns search_general_gtab;
#undef ROX_SEARCH_DECL

}  // namespace rox
