// rox_system.hpp -- private to the host units that work on a rox_system (roxtrace.hip, launch.hip,
// trace_entries.hip, focus.hip, search_entries.hip): the system, its per-stream state, and what
// those units call in each other.  Each group of StreamCtx belongs to the unit named above it.
#pragma once

#include <mutex>
#include <vector>

#include "rox_args.hpp"
#include "rox_host.hpp"

namespace rox {

constexpr char kHipWhere[] = "";        // (HIP_TRY: the messages of these units name no entry)
inline int (&fail)(int code, const char *fmt, ...) = host_fail;

// ---- per-stream state, by owner

// trace_entries.hip prepare_grid: pupil axes [2][cap] + the grid definition they currently hold
// (spot diagrams reuse one grid definition for every field and wavelength: the serial accumulate
// is skipped when unchanged)
struct AxesCache {
    double *d = nullptr;
    int32_t cap = 0;
    double key[4] = {0, 0, 0, 0};
    int32_t num = 0;
};

// launch.hip, HITS_COMPACT: tile states of the decoupled look-back, ticket, running base
struct CompactState {
    uint64_t *d_tiles = nullptr;
    int64_t tiles_cap = 0;
    uint32_t *d_ticket = nullptr;       // [0] ticket, [1] workgroups done
    int64_t *d_hits_base = nullptr;     // [2] running totals between launches (ping-pong)
    uint32_t epoch = 0;
};

// launch.hip, two-pass packed hits: the plain HITS launch's (x, y)[2][cap] and status[cap]
// (grow-only; launches on one stream run in order, so they share it)
struct PackScratch {
    double *d_xy = nullptr;
    uint8_t *d_status = nullptr;
    int64_t cap = 0;
};

// trace_entries.hip, ROX_HOST_POINTERS staging: HBM arena for big batches, device-mapped pinned
// block for small ones (grow-only)
struct StageArena {
    char *d = nullptr, *h = nullptr;
    size_t d_cap = 0, h_cap = 0;
};

// trace_entries.hip rox_trace_pupil_grids: the launch items of a batch of MORE than kInlineItems
// items (smaller batches travel in the kernel argument, rox_args.hpp BatchArgs).  Written into
// one of kSlots pinned slots (a slot is reused only after the copy that read it has completed),
// copied to d_items in stream order, read by the kernel through scalar loads.
struct BatchItems {
    static constexpr int kSlots = 4;
    TraceArgs *d_items = nullptr, *h_items = nullptr;
    int32_t cap = 0;
    std::vector<char> last;             // the bytes d_items holds (or is about to, in stream order)
    hipEvent_t ev[kSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_live[kSlots] = {false, false, false, false};
    uint32_t slot = 0;
    uint32_t *d_tickets = nullptr;      // HITS_COMPACT in a batch: [items][2] tickets
    uint64_t *d_tiles = nullptr;        // ... and [items][tiles] look-back states
    int64_t tickets_cap = 0, tiles_cap = 0;
    uint32_t epoch = 0;
};

// focus.hip rox_trace_through_focus[_grids] (grow-only): the device block -- the pupil axes, then
// items, planes and axis parameters (copied in one transfer from the pinned block h: the caller's
// arrays may be pageable and are free to go when the call returns), the statistics and the
// partial records of one launch
struct FocusBlock {
    char *d = nullptr;
    size_t cap = 0;
    Staging h;
    // ... the axis parameters and num of the axes at the head of the block (none after a regrow):
    // a call that repeats them byte for byte does not walk the axes again
    std::vector<double> prm;
    int32_t num = 0;
};

// Per-stream launch scratch.  Launches on one stream run in stream order, so
// they may share it; two streams (or two host threads on two streams) get two
// contexts, looked up under rox_system::mu.
struct StreamCtx {
    hipStream_t stream = nullptr;
    AxesCache axes;
    CompactState compact;
    PackScratch pack;
    StageArena stage;
    BatchItems batch;
    FocusBlock focus;
    // Everything a pupil-grid call does between reading / rewriting the cached axes
    // (prepare_grid) and handing its launches to the stream is one critical section per
    // stream: two host threads enqueueing on the SAME stream take turns (their launches run
    // in stream order anyway); different streams have different contexts and do not meet.
    std::mutex enqueue_mu;
    std::mutex batch_mu;                // one batch enqueue at a time per stream
    std::mutex stage_mu;                // one ROX_HOST_POINTERS call at a time per stream
    std::mutex compact_mu;              // epoch / ticket state: one HITS_COMPACT enqueue at a time
    std::mutex ticket_mu;               // first allocation of d_ticket / d_hits_base
};

}  // namespace rox

struct rox_system {
    int device = 0;
    int32_t n_ifcs = 0, n_wvls = 0;
    std::vector<rox_surface> rows;      // host copy (immutable)
    double *d_rows = nullptr;
    double *d_ntab = nullptr;
    double *d_phc = nullptr;            // [W][N][kPhaseConsts]
    double *d_wvls = nullptr;
    int32_t *d_slots[2] = {nullptr, nullptr};   // [0]: no phantom filtering, [1]: filtered
    int32_t n_seg[2] = {0, 0};
    int num_cus = 256;
    int features = 0;                   // F_* of the table
    int n_newton = 0;                   // interfaces intersected by Newton iteration
    std::mutex mu;                      // guards ctxs
    std::vector<rox::StreamCtx *> ctxs;
    // the small synchronous search entries (aiming, pupil search, vignetting, pupil
    // iterations): one device-mapped pinned block the kernel reads its problems from and
    // writes its answers to -- no allocation, no copy-engine transfer per call (round 4; a
    // call used to be hipMalloc + three hipMemcpyAsync + hipFree around a 10-300 us kernel)
    char *h_search = nullptr;
    size_t h_search_cap = 0;
    std::mutex search_mu;
};

namespace rox {

// ---- roxtrace.hip
// the context of (sys, st), made on first use, in cx; ROX_E_NOMEM when it cannot be made
int stream_ctx(rox_system *sys, hipStream_t st, StreamCtx *&cx);
// the lock of StreamCtx::enqueue_mu; empty when the context cannot be made (the call then fails
// in prepare_grid with the same condition)
std::unique_lock<std::mutex> enqueue_lock(rox_system *sys, hipStream_t st);

// ---- launch.hip
constexpr size_t kLdsLimit = 160 * 1024 - 64;      // of a workgroup
bool force_gtab();
int64_t rays_per_launch();
int blocks_per_cu(int bs);
int compact_blocks_per_cu();
int32_t compact_small_want(const rox_system *sys, int64_t n_rays);
bool want_small(const rox_system *sys, int64_t total_rays, int out_mode, int feat, int64_t n_items = 1);
int32_t full_tile_group(bool small);
int check_opts(const rox_system *sys, const rox_opts *o, const rox_out *out, int64_t n_rays);
int check_field(const rox_field *fld);
const TraceInstanceFns &trace_fns(int inst, const LaunchCfg &k);
int launch_setup(rox_system *sys, TraceArgs &a, int gen, bool prw, hipStream_t st, LaunchCfg &k, int &inst);
int launch(rox_system *sys, TraceArgs &a, int gen, hipStream_t st);

// ---- trace_entries.hip
// the checks of a pupil-grid launch and its arguments, the pupil axes aside (nothing enqueued)
int grid_args(rox_system *sys, const rox_field *fld, const rox_grid *grid, int32_t wvl_idx,
              const rox_opts *opts, const rox_out *out, TraceArgs &a);

}  // namespace rox
