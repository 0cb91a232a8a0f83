// launch.hip -- the launch policy of the trace kernels and the launch itself: the checks of
// rox_opts / rox_out, which instance, workgroup size, grid and LDS a launch gets, the per-stream
// HITS_COMPACT and pack state, the chunk loop (declared in rox_system.hpp).
#include <atomic>
#include <climits>

#include "rox_system.hpp"
#include "../../include/roxtrace_diag.h"

namespace rox {

// A table that does not fit the LDS of a workgroup (~220 interfaces at 736 B a row) is traced
// by the general instance that leaves it in global memory and reads it with scalar loads
// (F_GTAB; bit-identical, every output mode): SequentialModel has no size limit either.
// ROX_FORCE_GTAB=1 sends every launch there, the search kernels' included (tests; read once).
bool force_gtab()
{
    static const bool v = env_flag("ROX_FORCE_GTAB");
    return v;
}

// The LDS need of a launch of instance `inst` (rox_kernel.hpp trace_tiles), the packed-hits stash
// included.  gtab: the general instance over a table in global memory; otherwise gtab_of() says
// where the instance reads it.  There the clear-aperture thresholds get an array instead.
static size_t launch_lds(const rox_system *s, int inst, bool per_ray_wvl, bool fast, bool gtab, int out_mode)
{
    const int feat = kInstances[inst];
    // (an instance compiled with F_PHASE stages the phase constants, needed or not)
    const bool phase = gtab || (feat & F_PHASE), aplist = gtab || (feat & F_APLIST);
    const bool global_table = gtab || gtab_of(feat, fast, out_mode) != 0;
    const size_t N = s->n_ifcs, Wn = per_ray_wvl ? (size_t)s->n_wvls : 1;
    size_t b = (global_table ? 0 : N * sizeof(dev_surface)) + Wn * N * sizeof(double) +
               ((phase && !global_table) ? Wn * N * kPhaseConsts * sizeof(double) : 0) +
               ((global_table && aplist) ? N * ROX_MAX_AP * sizeof(double) : 0) +
               ((size_t)s->n_wvls + N) * sizeof(double) + 2 * N * sizeof(int32_t);
    if (fast && !gtab)  // (mu, mu^2, sg) per (wavelength row, interface) behind the slot map
        b += Wn * 3 * N * sizeof(double);
    if (out_mode == ROX_OUT_HITS_COMPACT)       // two tiles of packed pairs (rox_kernel.hpp)
        b += 16 + 2 * 16 * (size_t)block_of(ROX_OUT_HITS_COMPACT, feat);
    return up16(b);
}

// ROX_FAST_FP64 is a permission, taken where it buys something: the reduced-output modes (bound
// by VALU issue) always, FULL packets where the system makes them VALU-bound too (below).
// ROX_FAST_FP64_DISABLE=1 (read once) ignores the flag everywhere: an A/B switch for callers
// that set it by default.
static bool use_fast(const rox_system *sys, const rox_opts &o)
{
    static const bool off = env_flag("ROX_FAST_FP64_DISABLE");
    // FULL packets: the tolerance-mode kernels write them too (trace_ray_fast), and the host sends
    // a launch there where that pays -- systems whose interfaces are mostly aspheres (the same
    // test that picks their FULL workgroup, want_small()): there the FULL kernel is bound by the
    // Spencer-Murty arithmetic (phone lens, 8 aspheres in 12: 265 -> 208-212 us per 2^20 rays).
    // Everywhere else FULL is bound by its stores, which the shorter arithmetic only bunches up
    // (double Gauss 190.9 -> 200.1, .zmx zoom 191.9 -> 197.3; Nikkor 447.7 -> 440.6, lithography
    // lens 675.6 -> 670.2): those launches keep the exact kernels -- bit-exact is within any
    // tolerance.  Never under ROX_FILTER_PHANTOMS (the late append of a filtered segment is not
    // in trace_ray_fast).  ROX_FAST_FP64_FULL=0 / 1 (read once): never / wherever possible (A/B).
    // (full_env: unset or empty -> -1, 0 -> 0, anything else -> 1; LLONG_MIN stands for unset)
    static const long long full_raw = env_int("ROX_FAST_FP64_FULL", LLONG_MIN);
    static const int full_env = full_raw == LLONG_MIN ? -1 : full_raw != 0;
    if (!(o.flags & ROX_FAST_FP64) || off)
        return false;
    if (o.out_mode != ROX_OUT_FULL)
        return true;
    if ((o.flags & ROX_FILTER_PHANTOMS) || full_env == 0)
        return false;
    return full_env == 1 || sys->n_newton * 4 > sys->n_ifcs - 1;
}

int check_opts(const rox_system *sys, const rox_opts *o, const rox_out *out, int64_t n_rays)
{
    if (!sys || !o || !out)
        return fail(ROX_E_ARG, "null argument");
    if (o->out_mode < ROX_OUT_FULL || o->out_mode > ROX_OUT_FAN)
        return fail(ROX_E_ARG, "bad out_mode %d", o->out_mode);
    if (o->out_mode == ROX_OUT_OPD || o->out_mode == ROX_OUT_FAN) {
        if (sys->n_ifcs < 3)
            return fail(ROX_E_ARG, "OPD output needs at least 3 interfaces");
        if ((o->flags & ROX_FILTER_PHANTOMS) && sys->n_seg[1] != sys->n_seg[0])
            return fail(ROX_E_UNSUPPORTED, "OPD output with filter_out_phantoms");
        if (!(o->wf.ref_radius != 0.0))
            return fail(ROX_E_ARG, "OPD output needs rox_opts.wf (ref_radius is 0)");
        if (o->wf.kind < ROX_WF_FINITE || o->wf.kind > ROX_WF_INF_SPLIT)
            return fail(ROX_E_ARG, "bad rox_wavefront.kind %d", o->wf.kind);
    }
    if (o->out_mode == ROX_OUT_HITS_COMPACT) {
        if (!out->n_hits)
            return fail(ROX_E_ARG, "HITS_COMPACT output needs rox_out.n_hits");
        if (o->flags & ROX_HOST_POINTERS)
            return fail(ROX_E_ARG, "HITS_COMPACT writes device or device-mapped pinned host "
                                   "memory directly: do not set ROX_HOST_POINTERS");
        // rox_out.ld = capacity of seg in (x, y) pairs.  A call that does not append can need
        // up to n_rays of them; an appending call is clamped by the kernel (n_hits < 0)
        if (!(o->flags & ROX_HITS_APPEND) && out->ld < n_rays)
            return fail(ROX_E_ARG, "HITS_COMPACT: out.ld (%lld pairs of room) < n_rays (%lld)",
                        (long long)out->ld, (long long)n_rays);
        if (out->ld < 0)
            return fail(ROX_E_ARG, "HITS_COMPACT: negative out.ld");
    } else if (out->ld < n_rays) {
        return fail(ROX_E_ARG, "out.ld (%lld) < n_rays (%lld)", (long long)out->ld, (long long)n_rays);
    } else if (o->flags & ROX_HITS_APPEND) {
        return fail(ROX_E_ARG, "ROX_HITS_APPEND goes with ROX_OUT_HITS_COMPACT only");
    }
    if (!out->seg && n_rays > 0)
        return fail(ROX_E_ARG, "out.seg is null");
    if ((o->flags & ROX_FILTER_PHANTOMS) && sys->rows[0].mode == ROX_PHANTOM)
        return fail(ROX_E_UNSUPPORTED, "phantom object surface with filter_out_phantoms");
    return 0;
}

int check_field(const rox_field *fld)
{
    if (!fld)
        return fail(ROX_E_ARG, "null argument");
    if (fld->kind < ROX_FLD_EPD || fld->kind > ROX_FLD_AIM_DIR)
        return fail(ROX_E_ARG, "bad rox_field.kind %d", fld->kind);
    return 0;
}

// workgroups per CU of a launch of `bs`-thread workgroups (the rest of the batch is
// grid-strided).  ROX_BLOCKS_PER_CU overrides it for experiments.
int blocks_per_cu(int bs)
{
    static const int v = (int)env_int("ROX_BLOCKS_PER_CU", 0);
    return v > 0 ? v : 32 * 256 / bs;      // measured: FULL 238 us at 8/CU, 228 us at 32/CU (256 threads)
}

// HITS_COMPACT: workgroups per CU.  Tiles are drawn by ticket, so any number of workgroups
// finishes the launch; a CU holds exactly one 1024-thread workgroup of these instances, and one
// persistent workgroup per CU that draws its four tiles in turn (table staged once, no
// workgroup start-up between tiles) measured 146 us per 2^20 rays into HBM against 159 us
// for one workgroup per tile (nine appended grids: 1.36 vs 1.49 ms; two per CU 1.40).
// ROX_COMPACT_BLOCKS_PER_CU overrides it for experiments.
int compact_blocks_per_cu()
{
    static const int v = (int)env_int("ROX_COMPACT_BLOCKS_PER_CU", 0);
    return v > 0 ? v : 1;
}

// HITS_COMPACT: how many first tickets take small tiles (rox_args.hpp compact_tiles).
// A launch that small tiles spread over no more workgroups than the chip has CUs (a
// 256 x 256 grid: 256 tiles of 256 rays instead of 64 of 1024) runs all of it that way:
// 30 vs 40 us into HBM, 41 vs 53 us into pinned memory.  Larger launches take full tiles
// throughout: small first tiles measured slower there (1024 x 1024: 178 vs 158 us into HBM,
// 319 vs 301 us into pinned memory; 45 x 1M rays of config 5: 26.3 vs 23.1 ms).
// ROX_COMPACT_SMALL_TILES overrides the count for experiments.
int32_t compact_small_want(const rox_system *sys, int64_t n_rays)
{
    static const int v = (int)env_int("ROX_COMPACT_SMALL_TILES", -1);
    if (v >= 0)
        return v;
    return n_rays <= (int64_t)sys->num_cus * kSmallTile ? sys->num_cus : 0;
}

// rays per kernel launch (lane byte offsets are 32-bit: at most 2^28).
// ROX_RAYS_PER_LAUNCH overrides it (tests exercise the chunked path with it).
int64_t rays_per_launch()
{
    static const int64_t v = [] {
        const long long n = env_int("ROX_RAYS_PER_LAUNCH", 0);
        return (n > 0 && n <= (1LL << 28)) ? (int64_t)n : (int64_t(1) << 28);
    }();
    return v;
}

// FULL packets: tiles per XCD run of the workgroup -> tile map (rox_args.hpp full_tile_map()).
// Measured (DESIGN.md section 3.1 "Stores", profiles/r17_full_placement.jsonl): with 32, a die's
// workgroups of one round of 1024-thread workgroups write one contiguous eighth of every
// packet row -- double Gauss 188.9 -> 182.1 us per 2^20 rays, .zmx zoom 192.0 -> 185.5,
// lithography lens 681 -> 662; 16, 64 and 128 gain less, 2 to 8 lose.  Launches in small
// workgroups (want_small(): they do not fill the chip several times over) keep the identity:
// BASELINE configs[3] measured 32.6 us as it is, 32.9 mapped.
// ROX_FULL_TILE_GROUP=<G> (read once; 0 = identity) sets the group of every FULL launch, small
// workgroups included (A/B runs, tests).
constexpr int32_t kFullTileGroup = 32;
int32_t full_tile_group(bool small)
{
    static const long long env = env_int("ROX_FULL_TILE_GROUP", -1);
    if (env >= 0)
        return (int32_t)(env > kMaxTileGroup ? kMaxTileGroup : env);
    return small ? 0 : kFullTileGroup;
}

// the leanest compiled instance that covers `need` (index into kInstances).
// ROX_FORCE_INSTANCE=<index> (experiments: what a richer instance costs on a plain table) is
// honoured when that instance covers the need.
static int pick_instance(int need)
{
    const int n = (int)(sizeof kInstances / sizeof kInstances[0]);
    static const int forced = (int)env_int("ROX_FORCE_INSTANCE", -1);
    if (forced >= 0 && forced < n && (need & ~kInstances[forced]) == 0)
        return forced;
    for (int i = 0; i < n; ++i)
        if ((need & ~kInstances[i]) == 0)
            return i;
    return n - 1;
}

// Workgroup size of a launch (rox_config.hpp block_of()), measured rule
// (profiles/r05_block_rule.jsonl, tools/block_rule_sweep.py):
//  * FULL packets (1024-thread workgroups, one per CU, whose waves write packet rows in step
//    -- worth 13-23 % of the store rate on launches that fill the chip): a launch of at most
//    four rounds of such workgroups that would leave >= 30 % of its CU-rounds idle -- 64
//    workgroups (256^2 rays: 75 %), BASELINE configs[3]'s 320 on 256 CUs (two rounds, 37.5 %)
//    -- runs in ROX_BLOCK_SMALL-thread workgroups instead,
//    five of which fit a CU (256^2: 49 -> 29 us, configs[3]: 43.6 -> 34.0 us per pass);
//  * the reduced-output modes (512-thread workgroups): small workgroups up to kSmallWavesPerCu
//    waves per CU (configs[3]: 25.8 -> 23.9 us, 3 x 256^2: 43 -> 37 us), equal beyond, 3 % worse
//    at 2^20 rays.
// ROX_SMALL_BLOCKS=0 / 1 forces one form, ROX_SMALL_WAVES_PER_CU moves the second threshold.
constexpr int kSmallWavesPerCu = 24;
bool want_small(const rox_system *sys, int64_t total_rays, int out_mode, int feat, int64_t n_items)
{
    static const int forced = (int)env_int("ROX_SMALL_BLOCKS", -1);
    static const int per_cu_env = (int)env_int("ROX_SMALL_WAVES_PER_CU", 0);
    const int per_cu = per_cu_env > 0 ? per_cu_env : kSmallWavesPerCu;
    if (forced == 0 || forced == 1)
        return forced == 1;
    if (out_mode == ROX_OUT_FULL) {
        const int64_t big = block_of(ROX_OUT_FULL, feat, false);
        if (big <= ROX_BLOCK_SMALL)
            return false;
        // Newton instances: a workgroup waits at every surface for its slowest wave, and the
        // iteration counts differ per wave.  Where aspheres are a minority of the interfaces
        // the large workgroup's packet rows still win (the .zmx zoom, one asphere in 12: 209
        // -> 192 us per 2^20 rays; Nikkor, 4 in 28: 471 -> 445); where they are most of the
        // system small workgroups out of step with each other do (phone lens, 8 in 12: 263
        // against 288 us).  profiles/r05_full_block_newton.txt.
        if ((feat & kFeatNewton) && sys->n_newton * 4 > sys->n_ifcs - 1)
            return true;
        const int64_t per_item = (total_rays / n_items + big - 1) / big;
        const int64_t wgs = per_item * n_items, cus = sys->num_cus;
        const int64_t rounds = (wgs + cus - 1) / cus;
        const int64_t idle = rounds * cus - wgs;
        return rounds <= 4 && idle * 10 >= 3 * rounds * cus;
    }
    return (total_rays + 63) / 64 <= (int64_t)sys->num_cus * per_cu;
}

// the entry points of trace instance kInstances[inst] -- or of its tolerance-mode twin, or of the
// general instance over a table in global memory -- as launch_setup chose in k.  Every launch
// of a trace kernel asks here (launch(), the batched entry, the through-focus entry), so this
// is where rox_diag_trace_launches counts them by form.
constexpr int kTraceForms = 32;      // (inst * 2 + fast) * 2 + small; inst 7 = the global-table general instance
static std::atomic<uint64_t> g_trace_launches[kTraceForms];
const TraceInstanceFns &trace_fns(int inst, const LaunchCfg &k)
{
    g_trace_launches[((k.gtab ? 7 : inst) * 2 + (k.fast ? 1 : 0)) * 2 + (k.small ? 1 : 0)]
        .fetch_add(1, std::memory_order_relaxed);
#define ROX_TRACE_FNS(name, FEAT) &trace_##name,
#define ROX_TRACE_FAST_FNS(name, FEAT) &trace_##name##_fast,
    static const TraceInstanceFns *const fns[] = {ROX_TRACE_INSTANCES(ROX_TRACE_FNS)};
    static const TraceInstanceFns *const fast[] = {ROX_TRACE_INSTANCES(ROX_TRACE_FAST_FNS)};
#undef ROX_TRACE_FNS
#undef ROX_TRACE_FAST_FNS
    return k.gtab ? trace_general_gtab : *(k.fast ? fast : fns)[inst];
}

// The stream context's HITS_COMPACT state: the ticket words (of the tiles and of the pack pass:
// launches of one stream run in order and each leaves them zero), the running base, and room
// for `tiles` look-back states.  (Initialisations are enqueued on the launch stream itself: a
// stream created with hipStreamNonBlocking is not ordered after NULL-stream memsets.)
static int ensure_compact(StreamCtx *cx, int64_t tiles, hipStream_t st)
{
    CompactState &c = cx->compact;
    std::unique_lock<std::mutex> g(cx->ticket_mu);
    if (!c.d_ticket) {
        uint32_t *t = nullptr;
        int64_t *b = nullptr;
        HIP_TRY(hipMalloc(&t, 2 * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(t, 0, 2 * sizeof(uint32_t), st));
        HIP_TRY(hipMalloc(&b, 2 * sizeof(int64_t)));
        HIP_TRY(hipMemsetAsync(b, 0, 2 * sizeof(int64_t), st));
        c.d_hits_base = b;
        c.d_ticket = t;
    }
    g.unlock();
    if (tiles > c.tiles_cap) {
        HIP_TRY(regrow_zeroed(c.d_tiles, c.tiles_cap, tiles, sizeof(uint64_t) * (size_t)tiles, st));
        c.epoch = 0;
    }
    return 0;
}

// Packed hits in two passes -- the unsynchronised HITS instance into a scratch, then the
// streaming pack kernel (csrc/pack.hip) -- instead of the fused tile-synchronous instance.
// The fused instance pays three workgroup barriers and a look-back per 1024-ray tile with
// one workgroup per CU; that is the cheaper form while a tile's waves finish together
// (shallow spherical systems) and while the destination sits behind PCIe (the pairs cross
// the link while later tiles are traced).  On deep tables and Newton instances the waves
// finish far apart and the plain HITS launch + a ~17 B/ray pack pass wins: measured
// crossover in profiles/r04_pack_crossover.jsonl (tools/pack_bench.py).
// ROX_PACK_TWO_PASS=0 / 1 forces one form (experiments, tests).
static std::atomic<uint64_t> g_two_pass_launches{0}, g_fused_pack_launches{0};
constexpr int64_t kTwoPassMinRays = 1 << 16;
constexpr int64_t kTwoPassChunk = int64_t(1) << 24;     // rays per launch of the two-pass form
static bool want_two_pass(int64_t n_rays, const void *dst)
{
    const long long forced = env_int("ROX_PACK_TWO_PASS", -1);     // (read per call: tests flip it)
    if (forced == 0 || forced == 1)
        return forced == 1;
    return n_rays >= kTwoPassMinRays && is_device(dst);
}

static int ensure_pack_scratch(StreamCtx *cx, int64_t rays, bool need_status)
{
    const int64_t want = (rays + 511) & ~int64_t(511);
    if (want > cx->pack.cap) {
        HIP_TRY(release(cx->pack.d_status, cx->pack.cap));      // (made again below, on demand)
        HIP_TRY(regrow(cx->pack.d_xy, cx->pack.cap, want, sizeof(double) * 2 * (size_t)want));
    }
    if (need_status && !cx->pack.d_status)
        HIP_TRY(hipMalloc(&cx->pack.d_status, (size_t)cx->pack.cap));
    return 0;
}

// the table pointers of a launch, the leanest kernel instance that covers this system and
// these options, and its LDS need
int launch_setup(rox_system *sys, TraceArgs &a, int gen, bool prw, hipStream_t st, LaunchCfg &k,
                 int &inst)
{
    a.rows = sys->d_rows;
    a.n_table = sys->d_ntab;
    a.ph_consts = sys->d_phc;
    a.wvls = sys->d_wvls;
    a.slots = sys->d_slots[(a.opts.flags & ROX_FILTER_PHANTOMS) ? 1 : 0];
    a.n_ifcs = sys->n_ifcs;
    a.n_wvls = sys->n_wvls;
    int need = sys->features;
    if ((a.opts.flags & ROX_FILTER_PHANTOMS) && sys->n_seg[1] != sys->n_seg[0])
        need |= F_PHFILT;
    k.gen = gen;
    k.per_ray_wvl = prw;
    k.small = false;
    k.n_inline = 0;
    k.fast = use_fast(sys, a.opts);
    k.out_mode = a.opts.out_mode;
    k.stream = st;
    inst = pick_instance(need);
    k.gtab = false;
    k.lds = launch_lds(sys, inst, prw, k.fast, false, a.opts.out_mode);
    if (k.lds > kLdsLimit || force_gtab()) {    // (see force_gtab())
        inst = (int)(sizeof kInstances / sizeof kInstances[0]) - 1;
        k.fast = false;
        k.gtab = true;
        k.lds = launch_lds(sys, inst, prw, false, true, a.opts.out_mode);
        if (k.lds > kLdsLimit)
            return fail(ROX_E_UNSUPPORTED, "%d interfaces x %d wavelengths need %zu B of LDS for their "
                                           "indices and thresholds alone (max %zu)",
                        sys->n_ifcs, prw ? sys->n_wvls : 1, k.lds, kLdsLimit);
    }
    return 0;
}

int launch(rox_system *sys, TraceArgs &a, int gen, hipStream_t st)
{
    if (a.opts.out_mode == ROX_OUT_HITS_COMPACT && a.n_rays == 0) {
        // nothing to trace: the count is still owed (appending nothing leaves it as it is)
        if (!(a.opts.flags & ROX_HITS_APPEND))
            HIP_TRY(hipMemsetAsync(a.out.n_hits, 0, sizeof(int64_t), st));
        return 0;
    }
    if (a.n_rays == 0)
        return 0;
    const bool prw = a.wvl_idx != nullptr;
    LaunchCfg k;
    int inst;
    ROX_TRY(launch_setup(sys, a, gen, prw, st, k, inst));
    // lane byte offsets are 32-bit: at most 2^28 rays per launch
    const int64_t total = a.n_rays;
    int64_t chunk_max = rays_per_launch();
    k.small = !prw && want_small(sys, total, a.opts.out_mode, kInstances[inst]);   // (per-ray-wavelength lists keep the regular kernels)
    a.tile_group = a.opts.out_mode == ROX_OUT_FULL ? full_tile_group(k.small) : 0;
    const bool compact = a.opts.out_mode == ROX_OUT_HITS_COMPACT;
    StreamCtx *cx = nullptr;
    bool two_pass = false;
    // two host threads enqueueing HITS_COMPACT launches on one stream take turns with the
    // stream's epoch / ticket / tile-state words (the launches themselves run in stream order)
    std::unique_lock<std::mutex> compact_lock;
    if (compact) {
        ROX_TRY(stream_ctx(sys, st, cx));
        compact_lock = std::unique_lock<std::mutex>(cx->compact_mu);
        const int tb = block_of(ROX_OUT_HITS_COMPACT, kInstances[inst]);
        two_pass = want_two_pass(total, a.out.seg);
        if (two_pass) {
            // the scratch of the two passes is 17 B per ray of one launch: launches of at most
            // kTwoPassChunk rays bound it (272 MiB) whatever the call's size; the running base
            // carries the packed order across the launches exactly as it does across 2^28-ray
            // chunks.  Should the scratch still not be had, the fused instance -- which needs
            // none -- takes the call.
            if (chunk_max > kTwoPassChunk)
                chunk_max = kTwoPassChunk;
            const int64_t per2 = total < chunk_max ? total : chunk_max;
            if (ensure_pack_scratch(cx, per2, a.out.status == nullptr) != 0) {
                (void)hipGetLastError();
                two_pass = false;
                chunk_max = rays_per_launch();
            }
        }
        const int64_t per = total < chunk_max ? total : chunk_max;
        a.small_tiles = two_pass ? 0 : compact_small_want(sys, per);
        ROX_TRY(ensure_compact(cx, two_pass ? (per + kPackTile - 1) / kPackTile
                                            : compact_tiles(per, a.small_tiles, tb), st));
    }
    const rox_out out0 = a.out;
    a.in_ld = total;
    // HITS_COMPACT: launch c reads its base from slot[(c + 1) & 1] and leaves the running total
    // in slot[c & 1]; the first launch starts from zero, or -- ROX_HITS_APPEND -- from the
    // caller's count, copied into slot[1] first (device or device-mapped host memory)
    const bool append = compact && (a.opts.flags & ROX_HITS_APPEND);
    if (append)
        HIP_TRY(hipMemcpyAsync(cx->compact.d_hits_base + 1, out0.n_hits, sizeof(int64_t), hipMemcpyDefault, st));
    int64_t n_launch = 0;
    for (int64_t base = 0; base < total; base += chunk_max, ++n_launch) {
        a.ray_base = base;
        a.n_rays = total - base < chunk_max ? total - base : chunk_max;
        if (compact) {
            a.tile_state = cx->compact.d_tiles;
            a.ticket = cx->compact.d_ticket;
            a.hits_base_in = (n_launch == 0 && !append) ? nullptr : cx->compact.d_hits_base + ((n_launch + 1) & 1);
            a.hits_total_out = (base + chunk_max >= total) ? out0.n_hits : cx->compact.d_hits_base + (n_launch & 1);
            a.epoch = ++cx->compact.epoch;
            a.out.status = out0.status ? out0.status + base : nullptr;
        } else {
            a.out.seg = out0.seg + base;
            a.out.op = out0.op ? out0.op + base : nullptr;
            a.out.status = out0.status ? out0.status + base : nullptr;
            a.out.fail_surf = out0.fail_surf ? out0.fail_surf + base : nullptr;
            a.out.pupil = out0.pupil ? out0.pupil + base : nullptr;
        }
        if (compact)
            (two_pass ? g_two_pass_launches : g_fused_pack_launches).fetch_add(1, std::memory_order_relaxed);
        if (two_pass) {
            // pass 1: the plain HITS instance of the same rays into the scratch rows
            TraceArgs h = a;
            h.opts.out_mode = ROX_OUT_HITS;
            h.opts.flags &= ~(uint32_t)ROX_HITS_APPEND;
            h.out.seg = cx->pack.d_xy;
            h.out.ld = cx->pack.cap;
            h.out.op = nullptr;
            h.out.fail_surf = nullptr;
            h.out.pupil = nullptr;
            h.out.n_hits = nullptr;
            h.out.status = out0.status ? out0.status + base : cx->pack.d_status;
            LaunchCfg kh = k;
            kh.out_mode = ROX_OUT_HITS;
            kh.lds = launch_lds(sys, inst, prw, kh.fast, k.gtab, ROX_OUT_HITS);
            const int hb = block_of(ROX_OUT_HITS, kInstances[inst], kh.small);
            int64_t hblocks = (a.n_rays + hb - 1) / hb;
            const int64_t hcap = (int64_t)sys->num_cus * blocks_per_cu(hb);
            kh.grid = dim3((unsigned)(hblocks > hcap ? hcap : hblocks));
            trace_fns(inst, kh).launch(kh, h);
            // pass 2: survivors to their final place, in ray order
            PackArgs p;
            p.status = h.out.status;
            p.xy = cx->pack.d_xy;
            p.ld = cx->pack.cap;
            p.n_rays = a.n_rays;
            p.tile_state = a.tile_state;
            p.ticket = a.ticket;
            p.hits_base_in = a.hits_base_in;
            p.hits_total_out = a.hits_total_out;
            p.epoch = a.epoch;
            p.dst = out0.seg;
            p.ld_dst = out0.ld;
            int64_t pblocks = (a.n_rays + kPackTile - 1) / kPackTile;
            const int64_t pcap = (int64_t)sys->num_cus * 2;
            launch_pack(p, (unsigned)(pblocks > pcap ? pcap : pblocks), st);
            continue;
        }
        // enough workgroups to fill 256 CUs several times over, grid-stride the rest
        const int bs = block_of(a.opts.out_mode, kInstances[inst], k.small);
        int64_t blocks = compact ? compact_tiles(a.n_rays, a.small_tiles, bs) : (a.n_rays + bs - 1) / bs;
        const int64_t cap = (int64_t)sys->num_cus * (compact ? compact_blocks_per_cu() : blocks_per_cu(bs));
        if (blocks > cap)
            blocks = cap;
        k.grid = dim3((unsigned)blocks);
        trace_fns(inst, k).launch(k, a);
    }
    a.n_rays = total;
    a.out = out0;
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace rox

// ---- include/roxtrace.h
// The row pitch of a packet buffer of n_rays rays: the ray count rounded up to 4 KiB plus
// kPadDoubles, an odd multiple of 2 KiB, so that the ~130 component rows a lane writes never
// lie a power of two bytes apart.  Measured under the shipped kernel at 1024 x 1024
// (profiles/r17_full_placement.jsonl): pads of 256 to 2304 doubles within 1 % of each other,
// 0 and 64 slower (1 % and 2 % under the tile map, 16 % and 10 % without it), 8448 2 to 7 % slower
// -- today's 256 stays.  The buffer never grows by more than max(256, n_rays / 16) doubles a
// row: a small ragged grid, where the rounding alone would, gets the largest pitch of whole
// 64-byte lines within that.
extern "C" int64_t rox_packet_ld(int64_t n_rays)
{
    constexpr int64_t kPadDoubles = 256;
    if (n_rays <= 0)
        return 1;
    const int64_t cap = n_rays / 16 > 256 ? n_rays / 16 : 256;
    const int64_t want = (n_rays + 511) / 512 * 512 + kPadDoubles;
    return want - n_rays <= cap ? want : (n_rays + cap) / 8 * 8;
}

// ---- include/roxtrace_diag.h
extern "C" int rox_diag_full_tile_map(int64_t n_tiles, int32_t group, int64_t grid, int32_t wg0,
                                      int64_t *tiles)
{
    if (n_tiles < 0 || n_tiles > INT32_MAX || group < 0 || group > rox::kMaxTileGroup || grid < 1 ||
        wg0 < 0 || (n_tiles > 0 && !tiles))
        return rox::fail(ROX_E_ARG, "rox_diag_full_tile_map: bad argument");
    for (int64_t wg = 0; wg < grid; ++wg)
        for (int64_t t = wg; t < n_tiles; t += grid)
            tiles[t] = rox::full_tile_map(t, n_tiles, group, (uint32_t)wg0 % rox::kXcds);
    return 0;
}

extern "C" int rox_diag_pack_launches(uint64_t counts[2])
{
    if (!counts)
        return rox::fail(ROX_E_ARG, "null argument");
    counts[0] = rox::g_fused_pack_launches.load();
    counts[1] = rox::g_two_pass_launches.load();
    return 0;
}

extern "C" int rox_diag_trace_launches(uint64_t *counts, int32_t n)
{
    if (!counts || n < 0)
        return rox::fail(ROX_E_ARG, "rox_diag_trace_launches: bad argument");
    for (int32_t i = 0; i < n; ++i)
        counts[i] = i < rox::kTraceForms ? rox::g_trace_launches[i].load(std::memory_order_relaxed) : 0;
    return 0;
}
