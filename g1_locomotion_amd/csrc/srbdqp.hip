// srbdqp.hip -- C-ABI of the batched SRBD convex-MPC QP engine (see include/srbdqp.h) and kernel dispatch.
// Host side: HIP runtime only (stream, workspace, events).  No CPU fallback of any kind.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <chrono>
#include <string>
#include <type_traits>
#include <utility>
#include <unordered_set>
#include <vector>

#include "srbdqp.h"
#include "srbdqp_common.hpp"
#include "srbdqp_mfma.hpp"
#include "srbdqp_compact.hpp"
#include "srbdqp_split.hpp"
#include "srbdqp_setup1.hpp"
#include "srbdqp_wrench.hpp"
#include "srbdqp_wrench_lat_ew.hpp"
#include "srbdqp_cascade.hpp"
#include "srbdqp_fleet.hpp"
#include "srbdqp_observer.hpp"
#include "srbdqp_cascade.h"
#include "srbdqp_aql.hpp"

using srbdqp::KArgs;

// An optional per-QP device array, indexed by the caller's QP index: what the solves read (null: not set) and for how many QPs, and the library's own device
// copy of a host array (the host setters) with its capacity in elements
template <typename T>
struct PerQp {
    const T* dev = nullptr;
    size_t len = 0;
    T* own = nullptr;
    size_t cap = 0;
    void clear() { dev = nullptr; len = 0; }
    void release() { if (own) (void)hipFree(own); }
};

struct Carver {
    char* base; size_t off = 0;
    explicit Carver(char* b) : base(b) {}
    template <typename T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~size_t(255);
        return p;
    }
};

// ---- what a solve that restarts by further LAUNCHES needs beside its arguments: one structure for a handle's launch streams and for a ragged object ----
// RestartSet: the buffers through which a pass hands over to the one behind it.  RestartBufs: an owner's sets, carved from one allocation (carve_restart_sets) -- one
// set, or kRestartSets in rotation under SRBDQP_FLAG_DEFER_TAIL, where the passes of a solve run on a tail stream beside the owner's next solves.  Tail: such a
// stream with the event that closes each set's passes on it -- a set is reused only behind the event that closed its last user's passes (tail_wait).
constexpr int kRestartSets = 3;
struct RestartSet {
    float* resid = nullptr;                   // [items][4]: fp32 maxima of the last check of the QPs a pass left at its cap
    double* ybuf = nullptr;                   // [duals]: y when the caller passes none (a pass warm-starts from the outputs of the one before it)
    int32_t* stbuf = nullptr;                 // [items]: status when the caller passes none
    double* rho[2] = {nullptr, nullptr};      // [items] each: the rho a restart pass ran its QPs with, for the pass behind it (alternating)
    // index lists, [items] each, and their counters.  A launch stream under the defer flag: list[p] holds the QPs pass p left at its cap (cnt[p] of them), the
    // dispatch order of pass p + 1.  A ragged object: list[0] is the call's bucket permutation, list[1] its row offsets.
    int32_t* list[4] = {nullptr, nullptr, nullptr, nullptr}; int32_t* cnt = nullptr;
};
struct RestartBufs {
    char* mem = nullptr; size_t bytes = 0;
    size_t items = 0, duals = 0; int nsets = 0;   // the sets, and what each holds: QPs and dual doubles (a launch stream: B x 20 N; a ragged object: 20 per horizon row)
    RestartSet set[kRestartSets];
    double* ubuf = nullptr;                   // staged first pass: device copy of u for the pass behind it (KArgs::u_dev)
    bool fits(size_t n, size_t d, int sets) const { return mem && items >= n && duals >= d && nsets >= sets; }
};
struct Tail {
    hipStream_t st = nullptr;                 // highest priority, non-blocking
    hipEvent_t close[kRestartSets] = {nullptr, nullptr, nullptr};   // behind the last pass of the last solve that used set k on this stream
    bool used[kRestartSets] = {false, false, false};
    hipEvent_t last = nullptr;                // closes the passes of the last deferred solve on this stream (srbdqp_flush / srbdqp_ragged_flush wait for it), or null
};

struct srbdqp_handle {
    srbdqp_config cfg;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mid = nullptr;   // ev_mid: between the two kernels of the split pipeline
    bool ev_valid = false, ev_mid_valid = false;
    // device workspace for the host-buffer API
    char* ws = nullptr;
    size_t ws_bytes = 0;
    std::string err;
    const char* kname = "none";
    long long* stamps = nullptr;   // diagnostic stamp buffer (device), see srbdqp_set_stamp_buffer
    const int32_t* sched_hint = nullptr;   // device: previous step's iters[] (srbdqp_set_schedule_hint)
    size_t sched_hint_len = 0;             // its length: batches larger than that are dispatched in natural order
    // per-launch-stream device scratch (a caller may pipeline solves of one handle over several streams: each stream
    // needs its own dispatch order and its own split-pipeline hand-over workspace)
    struct StreamSlot {
        hipStream_t st = nullptr; bool used = false;
        int32_t* perm = nullptr; size_t perm_cap = 0;
        double* ws = nullptr; size_t ws_doubles = 0;
        // rho restart by further launches: this stream's sets (one; three once a solve deferred its passes: solve_deferred_passes), their rotation and the tail
        // stream the deferred passes run on.  An in-stream solve uses set 0.
        RestartBufs rb;
        unsigned long long rs_k = 0;
        Tail rtail;
        hipEvent_t ev_main = nullptr;      // behind a deferred solve's first pass: the tail stream waits for it
        // deferred tails (SRBDQP_FLAG_DEFER_TAIL): three rotating lists of continuation records and their counts
        char* tail = nullptr; int32_t* tail_cnt = nullptr; size_t tail_cap = 0;
        unsigned long long tail_k = 0;     // launches so far: list k % 3 is appended to, (k + 2) % 3 read, (k + 1) % 3 zeroed
        static constexpr int kTailHist = 8;
        long long tail_hist[kTailHist] = {0, 0, 0, 0, 0, 0, 0, 0};   // batch sizes of the last launches on this stream, newest first (bounds the records a launch can find)
        bool tail_live = false;            // records may be pending (a solve since the last flush)
    };
    static constexpr int kMaxSlots = 8;
    StreamSlot slots[kMaxSlots];
    // low-latency staging: one pinned, GPU-mapped slab carved into the arrays of srbdqp_stage
    char* stage_host = nullptr;
    char* stage_dev = nullptr;
    srbdqp_stage stage_h{};        // host addresses
    srbdqp_stage stage_d{};        // device addresses of the same memory
    // completion word of the staged path (last 64 bytes of the slab) + device counter of finished workgroups
    volatile int32_t* done_host = nullptr;
    int32_t* done_dev = nullptr;
    int32_t* done_count = nullptr;
    int32_t done_seq = 0;
    bool done_cs = false;          // the last launch publishes its completion word with the checksum of its outputs (KArgs::done_cs): wait_done() verifies it
    bool done_cs_x = false;        // ... which cover x_out
    // the staging array of each kind of side input a staged call can carry (ExtWrenchIn::staged, NormalsIn::staged), pinned and GPU-mapped like the slab; null
    // until the first call asks.  The wrench's is [capacity][N][6] (srbdqp_stage_ext_wrench), zero-filled; the normals' [capacity][N][12]
    // (srbdqp_stage_contact_normals), filled with (0, 0, 1): a block nobody wrote is no wrench / flat ground
    struct StagedSide { double* host = nullptr; double* dev = nullptr; };
    StagedSide staged_ext, staged_normals;
    int32_t prepared_B = 0; int prepared_maxs = 4; bool prepared_pcom = false;   // two-phase call: a set-up is pending, on the instantiation plan_two_phase chose
    // kernels whose dynamic-LDS limit has been raised on this handle's device (function attributes are per device, and a
    // process may hold handles on several)
    std::unordered_set<const void*> lds_attr_done;
    // the staged one-QP call's own AQL queue (srbdqp_aql.hpp); null: hipLaunchKernelGGL (set-up failed -- aql_why says how -- or SRBDQP_NO_AQL=1)
    srbdqp::AqlQueue* aql = nullptr;
    bool aql_tried = false;
    std::string aql_why;
    // the per-QP side inputs (one descriptor each below: RobotsIn, WeightsIn, NormalsIn, ExtWrenchIn).  The fp64 batch and ragged solves on the general kernel read them; null:
    // the config's robot / the config's q_diag and r_diag / flat ground for every QP
    PerQp<srbdqp_robot> robots;            // srbdqp_set_robots / _device
    PerQp<srbdqp_weights> weights;         // srbdqp_set_weights / _device
    PerQp<double> normals;                 // srbdqp_set_contact_normals / _device: [len][N][12] doubles (NormalsIn::per_qp), fp64 batch solves only
    PerQp<double> ext;                     // srbdqp_set_external_wrench / _device: [len][N][6] doubles (ExtWrenchIn::per_qp); a ragged bucket: the object's rows
    // SRBDQP_FLAG_ANY_HORIZON with a horizon that has no instantiation: cfg.horizon stays the live horizon n (every array has the caller's shape for n) and the
    // solves run the general kernel instantiated for live_nstar, the smallest tabulated horizon >= n, in its live-horizon mode (srbdqp_wrench.hpp, MODE = 3)
    int live_nstar = 0;                    // 0: the horizon has its own instantiations
    std::string live_name;                 // srbdqp_kernel_name of such a handle: wrench_f64_n<N*>_h<n>
    // the horizon buffers of srbdqp_fleet_rollout_*, for B robots, carved from one allocation; null until the first roll-out asks (ensure_fleet_buffers)
    struct FleetBufs {
        char* mem = nullptr; size_t bytes = 0, B = 0;
        double *x_ref = nullptr, *foot = nullptr, *pcom = nullptr, *landing = nullptr, *u = nullptr, *x_out = nullptr;
        uint8_t* contact = nullptr;
        int32_t *status = nullptr, *iters = nullptr;
        double* normals = nullptr;         // [B][N][12], carved only while a terrain is set: the contact normals of a terrain roll-out's solves (Call::side)
        unsigned flavour = 0;              // the roll-out flavours that have asked so far (kObserved | kSteered: ensure_fleet_buffers)
        // carved once an observed roll-out has asked: the external wrench of its solves (Call::side), [B][N][6], and the two-slot ring of states
        // [2][B][13] and footholds [2][B][12] the observer reads where the caller keeps no logs
        double *ew = nullptr, *ring_x = nullptr, *ring_feet = nullptr;
        // carved once a steered roll-out has asked: the heading every robot's next foot lands with, [B] (srbdqp_mpc_inputs_steered_* writes it)
        double* landing_yaw = nullptr;
        // carved once a previewed roll-out has asked: where foot holds a previewed point, [B][N][4] (srbdqp_mpc_inputs_previewed_* writes it)
        uint8_t* previewed = nullptr;
    } fleet;
    // the ground under the fleet (srbdqp_set_terrain, include/srbdqp_cascade.h): the library's device copy of the height map; map.h null: flat ground
    struct Terrain {
        srbdqp::TerrainMap map{};
        double* own = nullptr; size_t cap = 0;
    } terrain;
};

// slot of a launch stream (at most kMaxSlots distinct streams per handle; null when exhausted)
srbdqp_handle::StreamSlot* stream_slot(srbdqp_handle* h, hipStream_t st) {
    for (auto& s : h->slots) if (s.used && s.st == st) return &s;
    for (auto& s : h->slots) if (!s.used) { s.used = true; s.st = st; return &s; }
    h->err = "more than 8 distinct launch streams on one handle";
    return nullptr;
}

namespace {

// Longest-first dispatch order from the previous step's iteration counts (one workgroup; counting sort by iters/4,
// descending).  QPs that needed many ADMM iterations last time are started first, so the straggler tail of a launch
// overlaps the bulk instead of trailing it.  The hint only orders work; every QP is solved in full either way.
__global__ __launch_bounds__(1024) void srbdqp_schedule_kernel(const int32_t* iters_prev, int32_t* perm, int B) {
    __shared__ int cnt[128];
    __shared__ int base[128];
    const int t = threadIdx.x;
    if (t < 128) cnt[t] = 0;
    __syncthreads();
    for (int i = t; i < B; i += 1024) {
        int k = iters_prev[i] >> 2;
        k = k < 0 ? 0 : (k > 127 ? 127 : k);
        atomicAdd(&cnt[127 - k], 1);
    }
    __syncthreads();
    if (t == 0) { int acc = 0; for (int k = 0; k < 128; ++k) { base[k] = acc; acc += cnt[k]; } }
    __syncthreads();
    for (int i = t; i < B; i += 1024) {
        int k = iters_prev[i] >> 2;
        k = k < 0 ? 0 : (k > 127 ? 127 : k);
        perm[atomicAdd(&base[127 - k], 1)] = i;
    }
}

std::string g_create_err;

// a HIP call that must succeed; on failure o->err (a handle or a ragged object) names it
#define HIP_TRY(o, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (o)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return SRBDQP_E_HIP;                                                                 \
        }                                                                                        \
    } while (0)

// horizons with an instantiation (the 4-wave compact kernel: N in {4, 8, 10} with up to 4 stance contacts per step, N in
// {12, 16, 20} with at most 2; the one-wave kernel: <= 64 presolved variables; the general kernel: every horizon and pattern)
using Horizons = std::integer_sequence<int, 4, 8, 10, 12, 16, 20, 24>;

template <int... Ns>
constexpr bool horizon_in(int N, std::integer_sequence<int, Ns...>) { return ((N == Ns) || ...); }
bool horizon_supported(int N) { return horizon_in(N, Horizons{}); }

// smallest horizon with an instantiation that is >= n (0: none)
template <int... Ns>
constexpr int horizon_above(int n, std::integer_sequence<int, Ns...>) { int r = 0; ((r = (r == 0 && Ns >= n) ? Ns : r), ...); return r; }

// f(std::integral_constant<int, N>{}) for the handle's horizon N: the one place a run-time horizon becomes a template argument (a live horizon, SRBDQP_FLAG_ANY_HORIZON:
// the instantiation it runs on, N* -- only the general kernel's launcher and the refusals get that far)
template <class F, int... Ns>
int with_horizon_in(srbdqp_handle* h, F&& f, std::integer_sequence<int, Ns...>) {
    int rc = SRBDQP_E_INVALID;
    const int N = h->live_nstar ? h->live_nstar : h->cfg.horizon;
    if (!((N == Ns && ((rc = f(std::integral_constant<int, Ns>{})), true)) || ...)) h->err = "unsupported horizon";
    return rc;
}
template <class F>
int with_horizon(srbdqp_handle* h, F&& f) { return with_horizon_in(h, f, Horizons{}); }

// staged path, a multi-pass solve of which only the first pass ran: its arguments, how many restart passes may follow it, the set whose buffers they use
// (the host starts the next pass if a status asks for it)
struct Lazy {
    KArgs a1;
    int rcount = 1;
    const RestartSet* set = nullptr;
    bool pending = false;          // the solve really was such a first pass (not: restarted in place, or no restart at all)
};

// ---- which kernel a solve runs: a Plan, decided once per solve by plan_solve() (behind restart_iter_of) and executed by launch() and the launchers ----
enum class Family { Wave, WaveDefer, Split, Compact, General };   // one wave per QP, ... with deferred tails, the split pipeline, the 4-wave compact kernel, the general kernel
// General: any (kFormRows below has a row for each but Lat, the staged low-latency instantiation); Compact: Plain or Lat (the dump is a pass's a.mode == 1)
// (LatExtWrench: the low-latency instantiation of MODE 7, which only a staged wrench call -- Call::side -- plans; no handle state has its bit)
// (LatNormals: the same for MODE 4 and a staged normals call)
enum class Form { Plain, Robots, Weights, ExtWrench, Normals, Live, RankAware, Lat, LatExtWrench, LatNormals };
// the rho restart of restart_iter_of: none, inside the kernel, further launches on the caller's stream (the staged call: started by the host), or off that stream
// -- the next launch on it (WaveDefer) or a tail stream (solve_deferred_passes, the ragged buckets)
enum class Restart { Off, InPlace, Launches, Deferred };
struct Plan {
    Family family = Family::General;
    int maxs = 4;                  // the presolved families: the MAXS instantiation, 2 or 4 stance contacts per step
    Form form = Form::Plain;
    bool tile_classes = false;     // General, fp32: the first pass is split by tile precision
    bool wave_setup = false;       // Split: the set-up with one wave per QP (not SRBDQP_FLAG_SETUP4, at most 64 presolved variables)
    Restart restart = Restart::Off;
};

// The side input a call brings with it (the staged wrench and normals calls, the solves of an observed or a terrain roll-out), which every pass of the call reads
// in place of the handle's.  One kind or none: no instantiation reads two.  dev: the device address of the array, [B][N][6] or [B][N][12].  host: the host
// address of the same memory -- one staged QP carries the input in the argument segment, copied from there -- or null: the array is the device's alone and
// never goes inline.
enum class Side { None, ExtWrench, Normals };
struct CallSide {
    Side kind = Side::None;
    const double* dev = nullptr;
    const double* host = nullptr;
};

// what one call decides, on the caller's stack: every launch of the call -- restart passes included -- reads the same one, so a later pass runs the
// kernel the first one did (plan)
struct Call {
    bool f32 = false;              // the caller's buffers are float
    bool staged = false;           // srbdqp_solve_staged_f64 (with or without the completion word)
    bool signal = false;           // the launch publishes the completion word
    bool use_hint = false;         // the dispatch hint applies (it belongs to the device-buffer API)
    Lazy* lazy = nullptr;          // staged path: run only the first pass of a multi-pass solve and hand it back here
    CallSide side;                 // the side input of THIS call, if it brings one
    Plan plan;                     // plan_solve(h, c, B, ...), once the fields above are set
};

inline int maxs_or(const srbdqp_config& c, int fallback) { return c.max_contacts_per_step > 0 ? c.max_contacts_per_step : fallback; }

// stance contacts of B QPs' host-side flags: the most in one step, and the most presolved variables (3 per stance contact) of one QP.  !want_neff: stops
// once a step has more than 2 (all the instantiation choice needs)
struct Contacts {
    int worst = 0, neff = 0;
    int maxs() const { return worst <= 2 ? 2 : 4; }
};
Contacts scan_contacts(const uint8_t* c, size_t B, size_t N, bool want_neff) {
    Contacts r;
    for (size_t b = 0; b < B && (want_neff || r.worst <= 2); ++b) {
        int na = 0;
        for (size_t q = b * N; q < (b + 1) * N; ++q) {
            const int cnt = (c[4 * q] != 0) + (c[4 * q + 1] != 0) + (c[4 * q + 2] != 0) + (c[4 * q + 3] != 0);
            if (cnt > r.worst) r.worst = cnt;
            na += cnt;
        }
        if (3 * na > r.neff) r.neff = 3 * na;
    }
    return r;
}

// the bound on the stance contacts per step of a batch whose flags the host sees: the config's, or the batch's own
inline int host_maxs(const srbdqp_handle* h, const uint8_t* contact, size_t B) {
    return h->cfg.max_contacts_per_step > 0 ? h->cfg.max_contacts_per_step : scan_contacts(contact, B, (size_t)h->cfg.horizon, false).maxs();
}

// grow a device buffer to at least `want` elements (its contents are not kept); `busy`: a stream that may still use the old one
template <class O, class T>
int grow(O* o, T*& buf, size_t& cap, size_t want, hipStream_t busy, const char* what) {
    if (want <= cap) return SRBDQP_OK;
    if (busy) HIP_TRY(o, hipStreamSynchronize(busy));
    if (buf) HIP_TRY(o, hipFree(buf));
    buf = nullptr; cap = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf), want * sizeof(T));
    if (e != hipSuccess) { o->err = std::string(what) + ": " + hipGetErrorString(e); return SRBDQP_E_NOMEM; }
    cap = want;
    return SRBDQP_OK;
}

// (re)carve rb from one allocation: nsets sets for `items` QPs and `duals` dual doubles, `nlists` index lists per set (with their counters), u_doubles of ubuf.  The
// old contents are not kept: the caller has waited for everything that used them -- earlier work of this owner only -- and drained its tails (tail_drain).
template <class O>
int carve_restart_sets(O* o, RestartBufs& rb, size_t items, size_t duals, int nsets, int nlists, size_t u_doubles) {
    auto carve = [&](Carver c) {
        for (int i = 0; i < nsets; ++i) {
            RestartSet& r = rb.set[i];
            r.resid = c.take<float>(items * 4); r.ybuf = c.take<double>(duals); r.stbuf = c.take<int32_t>(items);
            r.rho[0] = c.take<double>(items); r.rho[1] = c.take<double>(items);
            for (int j = 0; j < nlists; ++j) r.list[j] = c.take<int32_t>(items);
            r.cnt = nlists ? c.take<int32_t>(16) : nullptr;
        }
        rb.ubuf = u_doubles ? c.take<double>(u_doubles) : nullptr;
        return c.off;
    };
    rb.items = rb.duals = 0; rb.nsets = 0;
    const int rc = grow(o, rb.mem, rb.bytes, carve(Carver(nullptr)), nullptr, "hipMalloc restart buffers");   // (a dry run for the size)
    if (rc != SRBDQP_OK) return rc;
    carve(Carver(rb.mem));
    rb.items = items; rb.duals = duals; rb.nsets = nsets;
    return SRBDQP_OK;
}

// ---- the tail-stream rotation of SRBDQP_FLAG_DEFER_TAIL (a launch stream has one Tail, a ragged object one per bucket) ----
template <class O>
int tail_create(O* o, Tail& t) {
    int least = 0, greatest = 0;
    HIP_TRY(o, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(o, hipStreamCreateWithPriority(&t.st, hipStreamNonBlocking, greatest));
    for (auto& ev : t.close) HIP_TRY(o, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return SRBDQP_OK;
}
void tail_destroy(Tail& t) {
    if (t.st) { (void)hipStreamSynchronize(t.st); (void)hipStreamDestroy(t.st); }
    for (auto ev : t.close) if (ev) (void)hipEventDestroy(ev);
}
// the set a solve takes: the next of the rotation, or the only one
inline int next_set(unsigned long long& k, int nsets) { return nsets > 1 ? (int)(k++ % (unsigned long long)nsets) : 0; }
// before anything on stream `on` overwrites set k: its last user on this tail has finished its passes
template <class O>
int tail_wait(O* o, const Tail& t, int k, hipStream_t on) { if (t.used[k]) HIP_TRY(o, hipStreamWaitEvent(on, t.close[k], 0)); return SRBDQP_OK; }
// behind the last pass of a solve on set k: its closing event, which a flush of the owner waits for too
template <class O>
int tail_close(O* o, Tail& t, int k) { HIP_TRY(o, hipEventRecord(t.close[k], t.st)); t.used[k] = true; t.last = t.close[k]; return SRBDQP_OK; }
// a flush: stream `on` waits for the passes of the last deferred solve
template <class O>
int tail_join(O* o, const Tail& t, hipStream_t on) { if (t.last) HIP_TRY(o, hipStreamWaitEvent(on, t.last, 0)); return SRBDQP_OK; }
// before the sets are carved anew: nothing is pending on the tail stream, no set has a last user
template <class O>
int tail_drain(O* o, Tail& t) {
    if (t.st) HIP_TRY(o, hipStreamSynchronize(t.st));
    t.last = nullptr;
    for (auto& u : t.used) u = false;
    return SRBDQP_OK;
}

int resolve_kernel(const srbdqp_config& c) {
    if (c.kernel == SRBDQP_KERNEL_WRENCH) return SRBDQP_KERNEL_WRENCH;
    return SRBDQP_KERNEL_COMPACT;   // AUTO, COMPACT, SPLIT and WAVE: the presolved family of srbdqp_compact.hpp
}

void fill_args(const srbdqp_config& c, KArgs& a) {
    a.max_iter = c.max_iter;
    a.check_every = c.check_every;
    a.dt = c.dt;
    a.inv_mass = 1.0 / c.mass;
    for (int i = 0; i < 3; ++i) a.iinv[i] = 1.0 / c.inertia[i];
    a.mu = c.mu;
    a.s = c.force_scale;
    a.fzmin_s = c.fz_min / c.force_scale;
    a.fzmax_s = c.fz_max / c.force_scale;
    for (int i = 0; i < 12; ++i) a.sqrtq[i] = std::sqrt(c.q_diag[i]);
    a.rs2 = c.r_diag * c.force_scale * c.force_scale;
    a.rho = c.rho;
    a.rho_eq = c.rho * c.rho_eq_scale;
    a.rho_fz = c.rho_fz_scale;
    a.sigma = c.sigma;
    a.alpha = c.alpha;
    a.eps_abs = c.eps_abs;
    a.eps_rel = c.eps_rel;
}

// arguments of a solve of B QPs: the config's constants and the inputs, everything else zero
KArgs base_args(const srbdqp_config& c, int32_t B, const void* x0 = nullptr, const void* x_ref = nullptr, const void* foot = nullptr,
                const uint8_t* contact = nullptr, const void* pcom = nullptr) {
    KArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_args(c, a);
    a.x0 = static_cast<const double*>(x0); a.xref = static_cast<const double*>(x_ref); a.foot = static_cast<const double*>(foot);
    a.contact = contact; a.pcom = static_cast<const double*>(pcom);
    a.B = B;
    return a;
}

template <typename K>
int set_lds_once(srbdqp_handle* h, K kernel, size_t lds) {
    const void* fn = reinterpret_cast<const void*>(kernel);
    if (!h->lds_attr_done.count(fn)) {
        HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        h->lds_attr_done.insert(fn);
    }
    return SRBDQP_OK;
}

// one launch through HIP: the kernel's dynamic-LDS limit (set_lds_once), the name srbdqp_kernel_name reports (nullptr: as it is), the launch, its error
template <typename K, typename... A>
int launch_kernel(srbdqp_handle* h, K kernel, const char* kname, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
    const int rc = set_lds_once(h, kernel, lds);
    if (rc != SRBDQP_OK) return rc;
    if (kname) h->kname = kname;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    HIP_TRY(h, hipGetLastError());
    return SRBDQP_OK;
}

// KERNEL_SPLIT (A/B): the one-wave set-up and the one-wave ADMM as two kernels with the hand-over through HBM.

template <int N, int MAXS>
int launch_split(srbdqp_handle* h, const Call& c, KArgs a, hipStream_t st) {
    using W = srbdqp::SplitWs<N, MAXS>;
    const size_t need = (size_t)a.B * W::doubles;   // indexed by QP, not by workgroup
    auto* slot = stream_slot(h, st);
    if (!slot) return SRBDQP_E_INVALID;
    int rc = grow(h, slot->ws, slot->ws_doubles, need, st, "hipMalloc split workspace");   // (a previous launch on this stream may still use the old buffer)
    if (rc != SRBDQP_OK) return rc;
    a.ws = slot->ws;
    h->prepared_B = 0;                                      // the split pipeline overwrites the workspace a pending two-phase set-up lives in
    constexpr size_t ldsA = srbdqp::CompactTraits<N, MAXS>::lds_bytes, ldsB = srbdqp::SplitSmem<N, MAXS>::bytes;
    rc = set_lds_once(h, &srbdqp::srbdqp_compact_kernel<N, MAXS, true>, ldsA);
    if (rc != SRBDQP_OK) return rc;
    static const std::string nm = "split_f64_n" + std::to_string(N) + "_s" + std::to_string(MAXS);
    h->kname = nm.c_str();
    bool wave_setup = false;                                 // set-up with one wave per QP (default where the QP fits one) or with four
    if constexpr (srbdqp::Setup1Smem<N, MAXS>::supported) if ((wave_setup = c.plan.wave_setup)) hipLaunchKernelGGL((srbdqp::srbdqp_setup1_kernel<N, MAXS, false>), dim3((unsigned)a.B), dim3(64), (srbdqp::Setup1Smem<N, MAXS>::bytes), st, a);
    if (!wave_setup) hipLaunchKernelGGL((srbdqp::srbdqp_compact_kernel<N, MAXS, true>), dim3((unsigned)a.B), dim3(srbdqp::kThreads), ldsA, st, a);
    if ((h->cfg.flags & SRBDQP_FLAG_TIMING) && !a.count_ptr) { HIP_TRY(h, hipEventRecord(h->ev_mid, st)); h->ev_mid_valid = true; }
    hipLaunchKernelGGL((srbdqp::srbdqp_admm_kernel<N, MAXS>), dim3((unsigned)a.B), dim3(64), ldsB, st, a);
    HIP_TRY(h, hipGetLastError());
    return SRBDQP_OK;
}

// Two-phase call (srbdqp_prepare_staged_f64 / srbdqp_solve_prepared_f64): the split pipeline's two kernels launched apart.
// phase 0 = set-up (+ dq/dx0) from a predicted x0, phase 1 = gradient patch for the measured x0 + ADMM + roll-out.
template <int N, int MAXS>
int launch_two_phase(srbdqp_handle* h, KArgs a, hipStream_t st, int phase) {
    if constexpr (srbdqp::Setup1Smem<N, MAXS>::supported && srbdqp::SplitWs<N, MAXS>::supported) {
        using W = srbdqp::SplitWs<N, MAXS>;
        const size_t need = (size_t)a.B * W::doubles;
        auto* slot = stream_slot(h, st);
        if (!slot) return SRBDQP_E_INVALID;
        if (need > slot->ws_doubles && phase == 1) { h->err = "srbdqp_solve_prepared_f64 without a matching srbdqp_prepare_staged_f64"; return SRBDQP_E_INVALID; }
        const int rc = grow(h, slot->ws, slot->ws_doubles, need, st, "hipMalloc split workspace");
        if (rc != SRBDQP_OK) return rc;
        a.ws = slot->ws;
        if (phase == 0) {
            constexpr size_t lds1 = srbdqp::Setup1Smem<N, MAXS>::bytes;
            hipLaunchKernelGGL((srbdqp::srbdqp_setup1_kernel<N, MAXS, false, false, true>), dim3((unsigned)a.B), dim3(64), lds1, st, a);
            static const std::string nm = "prepare_f64_n" + std::to_string(N) + "_s" + std::to_string(MAXS);
            h->kname = nm.c_str();
        } else {
            constexpr size_t ldsB = srbdqp::SplitSmem<N, MAXS>::bytes;
            a.defer_x0 = 1;
            hipLaunchKernelGGL((srbdqp::srbdqp_admm_kernel<N, MAXS>), dim3((unsigned)a.B), dim3(64), ldsB, st, a);
            static const std::string nm = "prepared_f64_n" + std::to_string(N) + "_s" + std::to_string(MAXS);
            h->kname = nm.c_str();
        }
        HIP_TRY(h, hipGetLastError());
        return SRBDQP_OK;
    } else {
        h->err = "the two-phase call needs at most 64 presolved variables (N <= 10 with <= 2 stance contacts per step, N = 4 with 4)";
        return SRBDQP_E_INVALID;
    }
}

int launch_two_phase_any(srbdqp_handle* h, const KArgs& a, hipStream_t st, int MAXS, int phase) {
    return with_horizon(h, [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (N <= 10) return MAXS == 2 ? launch_two_phase<N, 2>(h, a, st, phase) : launch_two_phase<N, 4>(h, a, st, phase);
        h->err = "the two-phase call is built for N in {4, 8, 10}";
        return SRBDQP_E_INVALID;
    });
}

// One wave per QP for the whole solve (srbdqp_setup1.hpp, FUSED): the default for large batches of the small
// instantiations; nothing but inputs and outputs touches HBM.
template <int N, int MAXS>
int launch_wave(srbdqp_handle* h, const Call& c, const KArgs& a, hipStream_t st) {
    constexpr size_t lds1 = srbdqp::Setup1Smem<N, MAXS>::bytes;
    static const std::string nm = "wave_f64_n" + std::to_string(N) + "_s" + std::to_string(MAXS);
    h->kname = nm.c_str();
    if (a.mode == 1) hipLaunchKernelGGL((srbdqp::srbdqp_setup1_kernel<N, MAXS, true, true>), dim3((unsigned)a.B), dim3(64), lds1, st, a);
    else if (c.plan.restart == Restart::InPlace) {   // the rho restart in place: (x, y) of a pass wait in [3][64] doubles behind the kernel's own LDS
        constexpr size_t ldsr = lds1 + 3 * 64 * sizeof(double);
        static_assert(8 * ((ldsr + 1279) / 1280) * 1280 <= 163840, "eight QPs per CU");
        hipLaunchKernelGGL((srbdqp::srbdqp_setup1_kernel<N, MAXS, true, false, false, true>), dim3((unsigned)a.B), dim3(64), ldsr, st, a);
    }
    else hipLaunchKernelGGL((srbdqp::srbdqp_setup1_kernel<N, MAXS, true>), dim3((unsigned)a.B), dim3(64), lds1, st, a);
    HIP_TRY(h, hipGetLastError());
    return SRBDQP_OK;
}

// The one-wave kernel with deferred tails (srbdqp_setup1.hpp, srbdqp_wave_defer_kernel): grid = tail workgroups (continuations of earlier launches on this
// stream, first) + one workgroup per QP of this launch.  a.B = 0: a flush launch (continuations only, one workgroup per record the lists can hold).
template <int N, int MAXS>
int launch_wave_defer(srbdqp_handle* h, KArgs a, hipStream_t st, srbdqp_handle::StreamSlot* slot) {
    constexpr size_t lds1 = srbdqp::Setup1Smem<N, MAXS>::bytes + 3 * 64 * sizeof(double);
    static_assert(8 * ((lds1 + 1279) / 1280) * 1280 <= 163840, "eight QPs per CU");
    static const std::string nm = "wave_defer_f64_n" + std::to_string(N) + "_s" + std::to_string(MAXS);
    h->kname = nm.c_str();
    const unsigned long long k = slot->tail_k++;
    a.tail_lists = slot->tail; a.tail_cnt = slot->tail_cnt; a.tail_cap = (int32_t)slot->tail_cap;
    a.tail_iout = (int32_t)(k % 3); a.tail_iin = (int32_t)((k + 2) % 3); a.tail_izero = (int32_t)((k + 1) % 3);
    // tail workgroups: one per record the list this launch reads CAN hold -- a bound the host knows without asking the device: a record was written by the launch
    // before this one on the stream, as a first pass that reached its mark (at most that launch's QPs) or as a continuation that reached another (at most the QPs
    // of the launches before it that may still re-balance): the sum of the last rho_restart_count batch sizes.  Workgroups without a record leave after one
    // scalar load; 8192 of them in front of a 4096-QP launch cost 0.7 % (16,384: 1.5 %, tools/defer_bench.py with SRBDQP_TAIL_WGS_MIN).  A first version sized
    // this from the record count the device reported through a host-mapped word and moved surplus records on to the next list: the report is stale by however
    // far the host runs ahead of the device, and with 95 % of every batch continuing and the host 300 launches ahead the lists overflowed (tools/defer_fuzz.py).
    long long T = 0;
    const int rmax = a.restart_max > 0 ? a.restart_max : 1;
    for (int j = 0; j < rmax && j < srbdqp_handle::StreamSlot::kTailHist; ++j) T += slot->tail_hist[j];
    if (T < 64) T = 64;
    static const long long tail_wgs_min = [] { const char* e = getenv("SRBDQP_TAIL_WGS_MIN"); return e ? atoll(e) : 0LL; }();   // (experiments: the cost of empty tail workgroups; read once)
    if (a.B > 0 && T < tail_wgs_min) T = tail_wgs_min;
    if (T > (long long)slot->tail_cap) T = (long long)slot->tail_cap;
    for (int j = srbdqp_handle::StreamSlot::kTailHist - 1; j > 0; --j) slot->tail_hist[j] = slot->tail_hist[j - 1];
    slot->tail_hist[0] = a.B;
    if (a.B == 0) for (auto& v : slot->tail_hist) v = 0;      // (a flush launch finishes every record in place: the lists are empty behind it)
    a.tail_wgs = (int32_t)T;
    const bool timing = (h->cfg.flags & SRBDQP_FLAG_TIMING) != 0;          // (srbdqp_last_kernel_ms: this launch, continuations of earlier solves included)
    if (timing) { HIP_TRY(h, hipEventRecord(h->ev0, st)); h->ev_mid_valid = false; }
    if (a.B > 0) hipLaunchKernelGGL((srbdqp::srbdqp_wave_defer_kernel<N, MAXS, false>), dim3((unsigned)(T + a.B)), dim3(64), lds1, st, a);
    else hipLaunchKernelGGL((srbdqp::srbdqp_wave_defer_kernel<N, MAXS, true>), dim3((unsigned)T), dim3(64), lds1, st, a);
    HIP_TRY(h, hipGetLastError());
    if (timing) { HIP_TRY(h, hipEventRecord(h->ev1, st)); h->ev_valid = true; }
    slot->tail_live = true;
    return SRBDQP_OK;
}

// SRBDQP_FLAG_DEFER_TAIL on the one-wave kernel: ONE instantiation per horizon for every launch and for the flush, whatever bound on the stance contacts a call came
// with -- a record written by a <4, 4> launch and continued by a <4, 2> one (the flush used to pick its MAXS from cfg.max_contacts_per_step, 0 -> 2, while the
// device API assumes 4 and the host API scans the flags per call) rebuilt the QP with the wrong bound and returned SRBDQP_CONTACT_BOUND with zero forces
constexpr int wave_defer_maxs(int N) { return N == 4 ? 4 : 2; }
int launch_wave_defer_any(srbdqp_handle* h, const KArgs& a, hipStream_t st, srbdqp_handle::StreamSlot* slot) {
    return with_horizon(h, [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (N <= 10) return launch_wave_defer<N, wave_defer_maxs(N)>(h, a, st, slot);
        h->err = "deferred tails exist for the one-wave kernel only (N <= 10, at most 2 stance contacts per step)";
        return SRBDQP_E_INVALID;
    });
}

// the handle's AQL queue, made at the first staged one-QP call (a 5 MB code object goes through the HSA loader once per process and device)
srbdqp::AqlQueue* aql_queue(srbdqp_handle* h) {
    if (h->aql_tried) return h->aql;
    h->aql_tried = true;
    const char* off = std::getenv("SRBDQP_NO_AQL");
    if (off && off[0] && off[0] != '0') { h->aql_why = "SRBDQP_NO_AQL is set"; return nullptr; }
    int bus = 0, dev = 0, dom = 0;
    if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, h->cfg.device) != hipSuccess || hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, h->cfg.device) != hipSuccess ||
        hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, h->cfg.device) != hipSuccess) { (void)hipGetLastError(); h->aql_why = "no PCI address for the HIP device"; return nullptr; }
    h->aql = srbdqp::AqlQueue::create(srbdqp::aql_device(dom, bus, dev), &h->aql_why);
    return h->aql;
}

// every kernel this handle started through its own queue has ended: before anything that must follow it is handed to a HIP stream
int aql_quiesce(srbdqp_handle* h) {
    if (!h->aql || !h->aql->in_flight()) return SRBDQP_OK;
    if (h->aql->wait_end(5000000000ull)) return SRBDQP_OK;
    h->err = "a kernel on the handle's AQL queue did not end within 5 s";
    return SRBDQP_E_HIP;
}

// (a word that came with a checksum -- KArgs::done_cs -- counts once the outputs read back agree with it: they travel without a fence in front of the word)
bool outputs_there(const srbdqp_handle* h) {
    if (!h->done_cs) return true;
    const size_t Nn = (size_t)h->cfg.horizon;
    const volatile uint64_t* u = reinterpret_cast<const volatile uint64_t*>(h->stage_h.u);
    uint64_t x = 0;
    for (size_t i = 0; i < 12 * Nn; ++i) x ^= u[i];
    if (h->done_cs_x) {
        const volatile uint64_t* xs = reinterpret_cast<const volatile uint64_t*>(h->stage_h.x);
        for (size_t i = 0; i < 13 * (Nn + 1); ++i) x ^= xs[i];
    }
    x ^= (uint64_t)(uint32_t)*reinterpret_cast<const volatile int32_t*>(h->stage_h.status) | ((uint64_t)(uint32_t)*reinterpret_cast<const volatile int32_t*>(h->stage_h.iters) << 32);
    // the records: {sequence number, how many records, XOR of one row of 16 lanes} every 16 bytes (srbdqp_common.hpp signal_done_checksum)
    const volatile int32_t* rec = h->done_host;
    const int32_t nrec = rec[1];
    if (nrec < 1 || nrec > 16) return false;
    for (int32_t r = 0; r < nrec; ++r) {
        if (rec[4 * r] != h->done_seq || rec[4 * r + 1] != nrec) return false;
        x ^= (uint64_t)(uint32_t)rec[4 * r + 2] | ((uint64_t)(uint32_t)rec[4 * r + 3] << 32);
    }
    return x == 0;
}

// the end of the last launch on the handle's stream: spin on its completion word (sequence number h->done_seq), or synchronise the stream
int wait_done(srbdqp_handle* h, bool spin) {
    if (spin) {
        const auto t0 = std::chrono::steady_clock::now();
        unsigned polls = 0;
        while (*h->done_host != h->done_seq || !outputs_there(h)) {
            if ((++polls & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
                // slow or failed launch: hand over to the runtime (reports a fault, or returns once the kernel is done)
                const int rq = aql_quiesce(h);
                if (rq != SRBDQP_OK) return rq;
                HIP_TRY(h, hipStreamSynchronize(h->stream));
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return SRBDQP_OK;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SRBDQP_OK;
}

// one workgroup of a *_kernel_in instantiation (arguments: KArgs, then StagedIn<N>) through the handle's own queue; false: the caller launches through HIP
template <class In>
bool aql_launch_in(srbdqp_handle* h, const Call& c, hipStream_t st, const char* kd_format, int n, int x, const KArgs& a, const In& in, unsigned block, size_t lds) {
    // (events and tail passes live on HIP streams; a call that does not spin on the completion word waits on its stream)
    if (!c.staged || st != h->stream || !a.done_flag || (h->cfg.flags & (SRBDQP_FLAG_DEFER_TAIL | SRBDQP_FLAG_TIMING | SRBDQP_FLAG_NO_SPIN))) return false;
    srbdqp::AqlQueue* q = aql_queue(h);
    if (!q) return false;
    char name[160];
    std::snprintf(name, sizeof(name), kd_format, n, x);
    const srbdqp::AqlKernel& k = srbdqp::aql_kernel(q->device(), name, sizeof(KArgs) + sizeof(In));
    return q->launch(k, &a, sizeof(KArgs), &in, sizeof(In), block, (uint32_t)lds);
}

// the one staged QP of a *_in launch whose host-visible outputs are u, x, status and iters in the staging arrays: completion word with their checksum, no fence
// (srbdqp_common.hpp signal_done_checksum; SRBDQP_DONE_FENCE=1 in the environment keeps the fence: A/B)
void staged_done_checksum(srbdqp_handle* h, KArgs& ai) {
    static const bool off = [] { const char* e = std::getenv("SRBDQP_DONE_FENCE"); return e && e[0] && e[0] != '0'; }();
    h->done_cs = false;
    if (off || !ai.done_flag || ai.B != 1 || ai.u_out != h->stage_d.u || ai.status != h->stage_d.status || ai.iters != h->stage_d.iters ||
        (ai.x_out && ai.x_out != h->stage_d.x) || (ai.y_out && !ai.y_capped_only)) return;
    ai.done_cs = 1;
    h->done_cs = true;
    h->done_cs_x = ai.x_out != nullptr;
}

// one staged QP whose inputs still sit in the library's own staging arrays: they ride in the kernel-argument segment (srbdqp_common.hpp StagedIn)
template <int N>
bool staged_inline_inputs(const srbdqp_handle* h, const Call& c, const KArgs& a, srbdqp::StagedIn<N>& in) {
    if (!(c.staged && a.B == 1 && a.x0 == h->stage_d.x0 && a.xref == h->stage_d.x_ref && a.foot == h->stage_d.foot && a.contact == h->stage_d.contact) ||
        a.perm || a.row_off || (a.pcom && a.pcom != h->stage_d.pcom)) return false;     // (a restart pass of the staged call too: the host starts it only for a QP at the cap)
    std::memcpy(in.x0, h->stage_h.x0, sizeof(in.x0));
    std::memcpy(in.xref, h->stage_h.x_ref, sizeof(in.xref));
    std::memcpy(in.foot, h->stage_h.foot, sizeof(in.foot));
    std::memcpy(in.contact, h->stage_h.contact, sizeof(in.contact));
    if (a.pcom) std::memcpy(in.pcom, h->stage_h.pcom, sizeof(in.pcom));
    return true;
}

// The staged low-latency door of the 4-wave and the general kernel: k_lat over the pass's grid, or -- one staged QP whose inputs ride in the argument segment --
// its *_kernel_in twin k_in through the handle's own AQL queue (code object: kd_format % (N, x)) or, failing that, through HIP.  Both kernels' LDS limits and the
// name BEFORE the AQL attempt, which needs none of them: HIP has loaded the kernels whichever way a later launch of this handle goes.
template <int N, typename KLat, typename KIn>
int launch_staged_lat(srbdqp_handle* h, const Call& c, const KArgs& a, hipStream_t st, KLat k_lat, KIn k_in, const char* kd_format, int x, unsigned block, size_t lds, const char* name) {
    srbdqp::StagedIn<N> in;
    if (a.count_ptr || a.tile_sel || !staged_inline_inputs<N>(h, c, a, in)) return launch_kernel(h, k_lat, name, dim3((unsigned)a.B), dim3(block), lds, st, a);
    if (const int rc = set_lds_once(h, k_lat, lds)) return rc;
    if (const int rc = set_lds_once(h, k_in, lds)) return rc;
    h->kname = name;
    KArgs ai = a; ai.inline_in = 1;
    staged_done_checksum(h, ai);
    if (aql_launch_in(h, c, st, kd_format, N, x, ai, in, block, lds)) return SRBDQP_OK;
    if (const int rc = aql_quiesce(h)) return rc;
    return launch_kernel(h, k_in, nullptr, dim3(1), dim3(block), lds, st, ai, in);
}

// The launchers execute c.plan: no cfg.kernel, no threshold and no side-input pointer chooses anything in them (the handle's arrays go on as kernel arguments).
// What a launcher still reads from the PASS's KArgs, because it differs between the passes of one solve:
//  * a.mode == 1: the assembly dump of the planned kernel (srbdqp_assemble_f64 / _wrench_f64 launch nothing else);
//  * the *_kernel_in twin of a _lat kernel (launch_staged_lat): !count_ptr, !tile_sel and staged_inline_inputs -- the pass's inputs are the staging arrays' own;
//  * an fp32 solve planned with tile classes splits its FIRST pass only (no resid_in, no count_ptr) and never a ragged bucket's (row_off): restart passes run
//    their few QPs on fp64 tiles in one launch; the two launches of the split carry tile_sel 1 and 2.
template <int N, int MAXS>
int launch_compact(srbdqp_handle* h, const Call& c, const KArgs& a, hipStream_t st) {
    const Plan& p = c.plan;
    if constexpr (srbdqp::Setup1Smem<N, MAXS>::supported) {
        if (p.family == Family::Wave) return launch_wave<N, MAXS>(h, c, a, st);
    }
    if constexpr (srbdqp::SplitWs<N, MAXS>::supported) {
        if (p.family == Family::Split) return launch_split<N, MAXS>(h, c, a, st);
    }
    constexpr size_t lds = srbdqp::CompactTraits<N, MAXS>::lds_bytes;
    static const std::string nm = "compact_f64_n" + std::to_string(N) + "_s" + std::to_string(MAXS);
    const dim3 grid((unsigned)a.B), block(srbdqp::kThreads);
    if (a.mode == 1)     // assembly dump: the same kernel, stopped before its factorisation
        return launch_kernel(h, &srbdqp::srbdqp_compact_kernel<N, MAXS, false, true>, nm.c_str(), grid, block, lds, st, a);
    if constexpr (MAXS == 2 && srbdqp::SplitWs<N, MAXS>::supported) {
        // staged batch-1 path (completion word): four waves for the set-up, then the one-wave iteration on wave 0 (srbdqp_compact.hpp, TAIL1) --
        // compiled for one workgroup's worth of registers.  tools/latency_patterns.py, tools/batch1_kernel_probe.py
        if (p.form == Form::Lat) {
            constexpr size_t lds1 = srbdqp::CompactTraits<N, MAXS>::lds_bytes_tail1;
            static_assert(lds1 <= 163840 && srbdqp::SplitWs<N, MAXS>::KS <= 64, "TAIL1: K^-1 rows behind the kernel's own LDS");
            static const std::string nml = nm + "_lat";
            return launch_staged_lat<N>(h, c, a, st, &srbdqp::srbdqp_compact_kernel<N, MAXS, false, false, true>, &srbdqp::srbdqp_compact_kernel_in<N, MAXS>,
                                        "_ZN6srbdqp24srbdqp_compact_kernel_inILi%dELi%dEEEvNS_5KArgsENS_8StagedInIXT_EEE.kd", MAXS, srbdqp::kThreads, lds1, nml.c_str());
        }
    }
    return launch_kernel(h, &srbdqp::srbdqp_compact_kernel<N, MAXS>, nm.c_str(), grid, block, lds, st, a);
}

// Horizons with a rank-aware instantiation (MODE = 5) of the general kernel: every tabulated one below 24 builds without scratch memory at the waves per SIMD of
// its MODE = 0 twin ("Rank-aware wrench steps", has the table); N = 24 -- whose MODE = 0 kernel keeps 20 bytes per lane there already -- has none.
constexpr int kRankAwareMaxHorizon = 20;
// Horizons whose general kernel has a per-QP-record instantiation (MODE = 2) without scratch memory: N = 24 has none -- the MODE = 0 kernel that ships keeps
// 20 bytes per lane in scratch with its three extra set-up waves, and a MODE = 2 copy without them (XW = 0) 24 bytes -- so the setters refuse an N = 24
// handle / a ragged object with an N = 24 bucket.  The MODE = 6 instantiation of the weights is the MODE = 2 one with one more LDS slot
// (DESIGN.md section 15), and the one of the normals (MODE = 4) has no N = 24 form either (section 13).
constexpr int kRobotsMaxHorizon = 20;

// ---- the forms of the general kernel: a handle's state (state_of), one row per form (kFormRows), which form a refusal names and which one a launch runs ----
// A handle's state is a SET of forms.  Live and RankAware are fixed by srbdqp_create, which refuses the two together; the four side inputs come and go with the
// setters -- a clearing call (NULL, 0) is accepted in every state, a setting one only beside the forms of its row's `beside` (check_handle, and for a ragged
// object every bucket's).  So robot records, weights and an external wrench combine, and nothing else does.  (srbdqp_ragged_create refuses
// SRBDQP_FLAG_RANK_AWARE, and a ragged object has no normals: its buckets are Plain, Live or any of records, weights and wrench.)
constexpr unsigned bit(Form f) { return 1u << (unsigned)f; }
struct FormRow {
    Form form;                     // (its state bit: bit(form))
    int mode;                      // the MODE of wrench_qp that its launches run (srbdqp_wrench.hpp, WrenchMode: the layout, the doubles behind it)
    const char* suffix;            // of the name a handle reports: wrench_f64_n<N><suffix> (Live: wrench_f64_n<N*><suffix><n>)
    const char* noun;              // a side input, as variant_check_batch names it; null: a form fixed by srbdqp_create
    unsigned beside;               // the forms that may be set beside it
    int max_horizon;               // the largest horizon with an instantiation
    const char* tail;              // behind "<call>: " in a refusal (include/srbdqp.h has the reasons and the lists; the texts are quoted in INTEGRATION.md and
};                                 // matched by the tests).  Live's has two %d: the handle's horizon and its instantiation's
constexpr FormRow kFormRows[] = {
    {Form::Plain, srbdqp::kModeSolve, "", nullptr, 0, 24, "refused"},            // (never refused: every call has the plain form)
    {Form::Robots, srbdqp::kModeRobots, "_rb", "per-QP robot records", bit(Form::Weights) | bit(Form::ExtWrench), kRobotsMaxHorizon,
     "refused while per-QP robot records are set (srbdqp_set_robots): only the fp64 batch and ragged solves on the general kernel read them -- one robot for "
     "every QP goes in srbdqp_config"},
    {Form::Weights, srbdqp::kModeWeights, "_wt", "per-QP cost weights (srbdqp_set_weights)", bit(Form::Robots) | bit(Form::ExtWrench), kRobotsMaxHorizon,
     "refused while per-QP cost weights are set (srbdqp_set_weights): only the fp64 batch and ragged solves on the general kernel read them -- one pair of "
     "weights for every QP goes in srbdqp_config"},
    {Form::ExtWrench, srbdqp::kModeExtWrench, "_ew", "an external wrench (srbdqp_set_external_wrench)", bit(Form::Robots) | bit(Form::Weights), kRobotsMaxHorizon,
     "refused while an external wrench is set (srbdqp_set_external_wrench): only the fp64 batch and ragged solves on the general kernel read it -- "
     "srbdqp_set_external_wrench(h, NULL, 0) goes back to no wrench"},
    {Form::Normals, srbdqp::kModeNormals, "_cn", "contact normals (srbdqp_set_contact_normals)", 0, kRobotsMaxHorizon,
     "refused while contact normals are set (srbdqp_set_contact_normals): only the fp64 batch solves on the general kernel read them -- "
     "srbdqp_set_contact_normals(h, NULL, 0) goes back to flat ground"},
    {Form::Live, srbdqp::kModeLive, "_h", nullptr, 0, 24,
     "refused on a handle whose horizon %d was admitted by SRBDQP_FLAG_ANY_HORIZON: only the fp64 batch, ragged and staged solves run a live horizon (the "
     "general kernel's fp64 batch instantiation for N = %d)"},
    {Form::RankAware, srbdqp::kModeRankAware, "_ra", nullptr, 0, kRankAwareMaxHorizon,
     "refused on a handle created with SRBDQP_FLAG_RANK_AWARE: only the fp64 batch and staged solves have rank-aware wrench steps (the general kernel's fp64 "
     "batch instantiation, flat ground, srbdqp_config's single robot)"},
};
constexpr const FormRow& row(Form f) { return kFormRows[(unsigned)f]; }
constexpr unsigned side_inputs() { unsigned s = 0; for (const FormRow& r : kFormRows) if (r.noun) s |= bit(r.form); return s; }
constexpr unsigned kSideInputs = side_inputs();
constexpr bool rows_in_order() { unsigned i = 0; for (const FormRow& r : kFormRows) if ((unsigned)r.form != i++) return false; return i == (unsigned)Form::Lat; }
static_assert(rows_in_order(), "row(f) indexes kFormRows by the enum");
static_assert(srbdqp::WrenchMode<row(Form::Robots).mode>::xd == 8 && srbdqp::WrenchMode<row(Form::Weights).mode>::xd == 10 && srbdqp::WrenchMode<row(Form::ExtWrench).mode>::xd == 11 &&
              srbdqp::WrenchMode<row(Form::Normals).mode>::xd == 0, "the doubles launch_side_form adds behind a form's layout: one more than the highest slot its mode writes");

// a handful of pointer and flag tests: no allocation, no string (srbdqp_solve_staged_f64, the batch-1 latency path, comes through here twice a call)
inline unsigned state_of(const srbdqp_handle* h) {
    return (h->robots.dev ? bit(Form::Robots) : 0u) | (h->weights.dev ? bit(Form::Weights) : 0u) | (h->ext.dev ? bit(Form::ExtWrench) : 0u) |
           (h->normals.dev ? bit(Form::Normals) : 0u) | (h->live_nstar ? bit(Form::Live) : 0u) | ((h->cfg.flags & SRBDQP_FLAG_RANK_AWARE) ? bit(Form::RankAware) : 0u);
}
// The two precedences over a state, which differ on purpose.  A REFUSAL names the oldest input present -- records, weights, wrench, normals, then the two forms of
// srbdqp_create -- so that a text a caller may match stays what it was when a later input learned to sit beside an earlier one.  The enum is in that order.
inline Form refusal_form(unsigned state) { return state ? (Form)__builtin_ctz(state) : Form::Plain; }
// A LAUNCH runs the form that reads the most: the two of srbdqp_create first (the handle has no other instantiation), then the wrench's kernel, which reads the
// weights and the records too (or their KArgs values), then the weights', which reads the records, then the records', then the normals'.
inline Form launch_form(unsigned state) {
    for (const Form f : {Form::RankAware, Form::Live, Form::ExtWrench, Form::Weights, Form::Robots, Form::Normals}) if (state & bit(f)) return f;
    return Form::Plain;
}

// `what` -- a C-ABI call by its name, or a kind of solve -- has no form for a handle with f in its state: the message and SRBDQP_E_INVALID
int refuse(srbdqp_handle* h, Form f, const char* what) {
    char tail[384];
    std::snprintf(tail, sizeof(tail), row(f).tail, (int)h->cfg.horizon, (int)h->live_nstar);
    h->err = std::string(what) + ": " + tail;
    return SRBDQP_E_INVALID;
}

// Which forms, besides Plain, each C-ABI call admits.  Every call below opens with require_form(h, "<its name>", <its set>); the fp64 batch solves (host, device,
// ragged) admit every form and have no set.  (Inside the general kernel's launcher a rank-aware or live handle further refuses the assembly dump and an fp32
// solve, which no entry point lets through; the ragged calls refuse an fp32 solve and robot records with a live bucket.)
// srbdqp_solve_staged_f64, srbdqp_update_f64 (a live handle passes here and not below: the staged solve runs its batch instantiation through the HIP launch)
constexpr unsigned kFormsStaged = bit(Form::Live) | bit(Form::RankAware);
// srbdqp_prepare_staged_f64, srbdqp_solve_prepared_f64 (a rank-aware handle passes: the one-wave kernels of the two-phase call have no wrench steps)
constexpr unsigned kFormsTwoPhase = bit(Form::RankAware);
// srbdqp_solve_batch_f32, srbdqp_solve_batch_device_f32
constexpr unsigned kFormsF32 = 0;
// srbdqp_assemble_f64 (a rank-aware handle passes: the dump of the compact kernels, which have no wrench steps)
constexpr unsigned kFormsAssemble = bit(Form::RankAware);
// srbdqp_assemble_wrench_f64
constexpr unsigned kFormsAssembleWrench = 0;
// the setter of side input f with an array (check_handle): in place of an earlier one, or beside what its row says.  The one exception: robot records pass the
// normals' set, because check_handle answers them in words of its own (kNormalsOnRobots)
constexpr unsigned forms_of_setter(Form f) { return bit(f) | row(f).beside | (f == Form::Normals ? bit(Form::Robots) : 0u); }
constexpr const char* kNormalsOnRobots = ": refused while per-QP robot records are set (srbdqp_set_robots): no instantiation reads both (DESIGN.md section 13)";

// the form a refusal would name against the set a call admits: integer tests on the way of a call that has the form; a string only when the refusal fires
inline int require_form(srbdqp_handle* h, const char* fn, unsigned forms) {
    const Form f = refusal_form(state_of(h));
    return (f == Form::Plain || (forms & bit(f))) ? SRBDQP_OK : refuse(h, f, fn);
}

// The general kernel (srbdqp_wrench.hpp): any contact pattern, fp64 or fp32 iterations / buffers.  Waves per SIMD of an instantiation over the layout L: what its
// LDS admits and the register budget, whichever is lower.  (Contact normals: the MODE = 0 layout + the table L, the budget of the MODE = 0 twin -- CHMAX is the
// same --; DESIGN.md section 13 has the table)
template <int N, typename R, int TB = 8, class L = srbdqp::WrenchSmem<N, TB>>
struct WrenchTraits {
    using S = L;
    static constexpr int by_lds = (S::lds_wgs * S::NW + 3) / 4 > 0 ? (S::lds_wgs * S::NW + 3) / 4 : 1;   // waves per SIMD LDS admits (rounded up: 3 workgroups of 3 waves put 3 waves on one SIMD)
    static constexpr int F32_ON_F64_WPS = 3;   // fp32 iterations on fp64 tiles, half rows longer than 30: 3 waves per SIMD with scratch beat 2 without any by 24 - 33 % (profiles/r05_f32_on_f64_tiles_wps.txt)
    static constexpr int F64_SMALL_WPS = 3;    // fp64, half rows up to 36 (N <= 12)
    static constexpr int want = (sizeof(R) == 4) ? ((TB == 8 && S::CHMAX > 30) ? F32_ON_F64_WPS : 3) : (S::CHMAX <= 36 ? F64_SMALL_WPS : (S::CHMAX <= 60 ? 2 : 1));   // register budget
    static constexpr int wps = by_lds < want ? by_lds : want;
};

// One launch of side-input form F of the general kernel (fp64 batch kernel, N <= 20): the kernel over the layout of F's mode at WPS waves per SIMD with the mode's
// doubles behind the layout, the name's suffix, the handle's arrays as further kernel arguments -- every launch of a solve (first pass, restart passes, deferred
// passes on the tail stream, ragged buckets) comes through here with this handle
template <int N, Form F, int WPS, typename K, typename... A>
int launch_side_form(srbdqp_handle* h, K kernel, const KArgs& a, hipStream_t st, const A&... arrays) {
    using S = srbdqp::WrenchLayout<N, row(F).mode>;
    constexpr int XD = srbdqp::WrenchMode<row(F).mode>::xd;
    constexpr size_t lds = S::bytes + XD * sizeof(double);
    constexpr int wgs = S::wgs_of(S::o_end + XD), by_lds = (wgs * S::NW + 3) / 4, by_waves = WPS * 4 / S::NW;   // (workgroups per CU and waves per SIMD the LDS admits; workgroups the waves admit)
    static_assert(lds <= 163840 && S::BT == srbdqp::WrenchSmem<N>::BT, "one QP must fit the LDS of a CU");
    static_assert((by_lds < WPS ? by_lds : WPS) == WPS && (wgs < by_waves ? wgs : by_waves) == (S::lds_wgs < by_waves ? S::lds_wgs : by_waves),
                  "the doubles behind the layout cost no wave per SIMD and no workgroup per CU");
    static const std::string nm = "wrench_f64_n" + std::to_string(N) + row(F).suffix;     // (one per instantiation)
    return launch_kernel(h, kernel, nm.c_str(), dim3((unsigned)a.B), dim3(S::BT), lds, st, a, arrays...);
}

template <int N, typename R, typename TIO>
int launch_wrench_t(srbdqp_handle* h, const Call& c, const KArgs& a, hipStream_t st) {
    using S = srbdqp::WrenchSmem<N>;
    constexpr int WPS = WrenchTraits<N, R>::wps;
    constexpr size_t lds = S::bytes;
    static_assert(lds <= 163840, "one QP must fit the LDS of a CU");
    // N = 24 on fp64 tiles holds ONE workgroup of 5 waves per CU (102 KB of LDS): three extra waves that take part in the set-up only
    // (45 tiles over 8 waves instead of 5; they end before the iterations) cost nothing the CU was using (round 3)
    constexpr int BXW = (N == 24) ? 3 : 0;
    using SB = srbdqp::WrenchSmem<N, 8, 5, BXW>;
    constexpr size_t ldsb = SB::bytes;
    static_assert(ldsb <= 163840, "one QP must fit the LDS of a CU");
    static const std::string nm = std::string("wrench_") + (sizeof(R) == 4 ? "f32" : "f64") + "_n" + std::to_string(N);
    const dim3 grid((unsigned)a.B);
    const Form form = c.plan.form;
    if (form == Form::RankAware) {
        // rank-aware wrench steps: the MODE = 5 instantiation of the fp64 batch kernel -- every launch of a solve (first pass, restart passes, deferred passes on the
        // tail stream, a dispatch order, the staged calls with their completion word) comes through here with this handle.  (srbdqp_create refuses the flag at
        // N = 24 and at a live horizon, and the entry points the fp32 and dump calls, robot records and contact normals.)  The layout of the MODE = 0 twin.
        if constexpr (sizeof(R) == 8 && N <= kRankAwareMaxHorizon) {
            if (a.mode == 1) return refuse(h, Form::RankAware, "the assembly dump");
            using S5 = srbdqp::WrenchLayout<N, row(Form::RankAware).mode>;
            static_assert(S5::bytes == lds && S5::BT == S::BT && WrenchTraits<N, double>::wps == WPS, "rank-aware steps cost no occupancy: the LDS and the waves per SIMD of the MODE = 0 twin");
            static const std::string nm_ra = nm + row(Form::RankAware).suffix;
            return launch_kernel(h, &srbdqp::srbdqp_wrench_ra_kernel<N, WPS>, nm_ra.c_str(), grid, dim3(S::BT), lds, st, a);
        } else return refuse(h, Form::RankAware, sizeof(R) == 4 ? "an fp32 solve" : "a solve at this horizon");
    }
    if (form == Form::Live) {
        // a live horizon n = cfg.horizon < N (SRBDQP_FLAG_ANY_HORIZON): the MODE = 3 instantiation of the fp64 batch kernel, n as its second argument -- every launch of
        // a solve (first pass, restart passes, deferred passes on the tail stream, ragged buckets, the staged calls with their completion word) comes through here
        // with this handle.  (The entry points refuse the fp32, dump and two-phase calls and the robot records on such a handle.)
        if constexpr (sizeof(R) == 8) {
            if (a.mode == 1) return refuse(h, Form::Live, "the assembly dump");
            // (the layout of the MODE = 0 twin -- the live horizon itself takes no LDS --, except N* = 24: four more entries of every lane's T^-1 half row in LDS
            //  instead of registers, srbdqp_wrench.hpp wrench_kreg64; still the twin's one workgroup per CU)
            using S3 = srbdqp::WrenchLayout<N, row(Form::Live).mode, 8, 5, BXW>;
            constexpr size_t lds3 = S3::bytes;
            static_assert(lds3 <= 163840 && S3::lds_wgs == SB::lds_wgs && (N == 24 || lds3 == ldsb), "a live horizon costs no workgroup per CU: the occupancy of the MODE = 0 twin");
            void (*k_live)(KArgs, int) = &srbdqp::srbdqp_wrench_kernel<N, double, double, row(Form::Live).mode, WPS, double, 5, BXW>;
            return launch_kernel(h, k_live, h->live_name.c_str(), grid, dim3(S3::BT), lds3, st, a, (int)h->cfg.horizon);
        } else return refuse(h, Form::Live, "an fp32 solve");
    }
    if (a.mode == 1) {
        if constexpr (sizeof(R) == 8) return launch_kernel(h, &srbdqp::srbdqp_wrench_kernel<N, double, double, srbdqp::kModeDump, WPS>, nm.c_str(), grid, dim3(S::BT), lds, st, a);
        else { h->err = "the assembly dump is fp64 only"; return SRBDQP_E_INVALID; }
    }
    if constexpr (sizeof(R) == 8 && N <= kRobotsMaxHorizon) {
        // The side-input forms, each by its row of kFormRows.  (The entry points refuse the staged, fp32 and dump calls while one is set, and the setters N = 24 and what
        // does not combine.)  The wrench's kernel takes the weights and the records too (or null: the KArgs values), the weights' the records (or null).  Contact
        // normals run on a layout (L, the frames' columns, is 288 N more bytes of LDS) and at waves per SIMD of their own (WrenchTraits over that layout).
        const double* const weights = reinterpret_cast<const double*>(h->weights.dev);
        const double* const robots = reinterpret_cast<const double*>(h->robots.dev);
        // (a staged wrench call -- no side input is set then, the entry points see to it -- brings the wrench of the call: the same kernel over the staged array)
        if (form == Form::ExtWrench) return launch_side_form<N, Form::ExtWrench, WPS>(h, &srbdqp::srbdqp_wrench_ew_kernel<N, WPS>, a, st, c.side.dev ? c.side.dev : h->ext.dev, weights, robots);
        if (form == Form::Weights) return launch_side_form<N, Form::Weights, WPS>(h, &srbdqp::srbdqp_wrench_wt_kernel<N, WPS>, a, st, weights, robots);
        if (form == Form::Robots) {
            void (*k_rb)(KArgs, const double*) = &srbdqp::srbdqp_wrench_kernel<N, double, double, row(Form::Robots).mode, WPS, double, 5, 0>;
            return launch_side_form<N, Form::Robots, WPS>(h, k_rb, a, st, robots);
        }
        if (form == Form::Normals) {
            constexpr int WPSN = WrenchTraits<N, double, 8, srbdqp::WrenchLayout<N, row(Form::Normals).mode>>::wps;
            // (a staged normals call -- no side input is set then, the entry points see to it -- brings the normals of the call: the same kernel over the staged array)
            return launch_side_form<N, Form::Normals, WPSN>(h, &srbdqp::srbdqp_wrench_cn_kernel<N, WPSN>, a, st, c.side.dev ? c.side.dev : h->normals.dev);
        }
    }
    if constexpr (sizeof(R) == 8 && N <= 10) {
        // staged batch-1 path (completion word): the low-latency instantiation -- two extra waves for the set-up (tables, T
        // assembly, tile phases) that end before the iterations, one workgroup's worth of registers (no scratch, V in
        // registers, every broadcast read of the T^-1 product in flight).  tools/latency_patterns.py
        if (form == Form::Lat) {
            constexpr int XW = (N >= 8) ? 2 : 1;
            using SL = srbdqp::WrenchSmem<N, 8, 5, XW>;
            static const std::string nm_lat = nm + "_lat";
            return launch_staged_lat<N>(h, c, a, st, &srbdqp::srbdqp_wrench_kernel<N, R, TIO, 0, 1, double, 5, XW>, &srbdqp::srbdqp_wrench_kernel_in<N, XW>,
                                        "_ZN6srbdqp23srbdqp_wrench_kernel_inILi%dELi%dEEEvNS_5KArgsENS_8StagedInIXT_EEE.kd", XW, SL::BT, SL::bytes, nm_lat.c_str());
        }
        // a staged wrench or normals call of a few QPs: the same waves and pipeline in MODE 7 (the wrench's rows for the roll-out behind the mode's slots) or in
        // MODE 4 (on the layout with the table L).  Through HIP on the caller's stream, every pass: the handle's own queue stays what it is.  One staged QP whose
        // inputs are the staging arrays' own: inputs and side input in the argument segment (the normals: 3,912 of its 4,096 bytes at N = 10), completion word
        // with the checksum (the *_in twin, as launch_staged_lat chooses it) -- unless the side input has no host address
        // The kernels and their launcher live in srbdqp_wrench_lat_ew.hip, a code object of their own: this one's text stays where it is without them.
        if (form == Form::LatExtWrench || form == Form::LatNormals) {
            const bool cn = form == Form::LatNormals;
            static const std::string nm_side[2] = {nm + "_lat" + row(Form::ExtWrench).suffix, nm + "_lat" + row(Form::Normals).suffix};
            srbdqp::StagedIn<N> in;
            const bool inl = !(a.count_ptr || a.tile_sel || !c.side.host || !staged_inline_inputs<N>(h, c, a, in));
            KArgs ai = a;
            if (inl) { ai.inline_in = 1; staged_done_checksum(h, ai); }
            // (one key per kernel -- N, kind, inline; no function lives at such an address)
            const bool first = h->lds_attr_done.insert(reinterpret_cast<const void*>(uintptr_t(16 * N + (cn ? 2 : 0) + (inl ? 1 : 0)))).second;
            h->kname = nm_side[cn].c_str();
            const hipError_t e = srbdqp::launch_wrench_side_lat(row(cn ? Form::Normals : Form::ExtWrench).mode, N, first, ai, inl ? &in : nullptr, c.side.host, c.side.dev, st);
            if (e != hipSuccess) { h->err = std::string("launch of ") + nm_side[cn] + ": " + hipGetErrorString(e); return SRBDQP_E_HIP; }
            return SRBDQP_OK;
        }
    }
    if constexpr (sizeof(R) == 4) {
        // fp32 iterations: QPs whose steps all have 0 or >= 3 stance contacts (every g coordinate a wrench coordinate,
        // cond(T) ~ 5e4) factor T in fp32 tiles -- half the LDS, one more workgroup per CU; a step kept in force
        // variables carries the conditioning of K (1e8) into T and needs fp64 tiles.  Two launches over the same grid,
        // each workgroup looks at its QP's contact flags and leaves at once if the QP belongs to the other launch.
        // Not on the staged path (its workgroups are counted: plan_solve), not in the restart pass (few QPs), not for ragged batches.
        if (c.plan.tile_classes && !a.count_ptr && !a.resid_in && !a.row_off) {
            using S4 = srbdqp::WrenchSmem<N, 4>;
            constexpr int WPS4 = WrenchTraits<N, R, 4>::wps;
            constexpr size_t lds4 = S4::bytes;
            KArgs a4 = a, a8 = a;
            a4.tile_sel = 1; a8.tile_sel = 2;
            const int rc = launch_kernel(h, &srbdqp::srbdqp_wrench_kernel<N, R, TIO, 0, WPS4, float>, nm.c_str(), grid, dim3(S::BT), lds4, st, a4);
            if (rc != SRBDQP_OK) return rc;
            return launch_kernel(h, &srbdqp::srbdqp_wrench_kernel<N, R, TIO, 0, WPS, double, 5, BXW>, nullptr, grid, dim3(SB::BT), ldsb, st, a8);
        }
    }
    return launch_kernel(h, &srbdqp::srbdqp_wrench_kernel<N, R, TIO, 0, WPS, double, 5, BXW>, nm.c_str(), grid, dim3(SB::BT), ldsb, st, a);
}

// the general kernel at the handle's horizon, on the call's element type
int launch_wrench(srbdqp_handle* h, const Call& c, const KArgs& a, hipStream_t st) {
    return with_horizon(h, [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if (c.f32) return launch_wrench_t<N, float, float>(h, c, a, st);
        return launch_wrench_t<N, double, double>(h, c, a, st);
    });
}

// one launch of the call's plan.  pass: 0 = the only launch of a solve, 1 = first of two (restart follows), 2 = second of two
int launch(srbdqp_handle* h, const Call& c, const KArgs& a, hipStream_t st, int pass = 0) {
    if (a.B <= 0) return SRBDQP_OK;
    const bool timing = (h->cfg.flags & SRBDQP_FLAG_TIMING) != 0;
    if (timing && pass != 2) { HIP_TRY(h, hipEventRecord(h->ev0, st)); h->ev_mid_valid = false; }
    int rc;
    if (c.plan.family == Family::General) rc = launch_wrench(h, c, a, st);
    else rc = with_horizon(h, [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (N <= 10) return (c.plan.maxs == 2) ? launch_compact<N, 2>(h, c, a, st) : launch_compact<N, 4>(h, c, a, st);
        else if constexpr (N <= 20) return launch_compact<N, 2>(h, c, a, st);
        else return SRBDQP_OK;     // (N = 24 never gets here: plan_solve)
    });
    if (rc != SRBDQP_OK) return rc;
    if (timing && pass != 1) {
        HIP_TRY(h, hipEventRecord(h->ev1, st));
        h->ev_valid = true;
    }
    return SRBDQP_OK;
}

// The arrays of a host-buffer call (a handle's or a ragged object's): in() one the call uploads, out() one it downloads, zeroed() one it clears first (and
// downloads, given a host pointer).  A null host pointer means no array, except for out(..., true): status / iters, which the kernels write either way.
struct HostIo {
    struct Arr { void* dev; const void* in; void* out; size_t bytes; bool zero; };
    Carver c;
    Arr arr[20];                   // (at most 12: solve_host_impl; 16: a tracked, observed roll-out with every log)
    int n = 0;
    explicit HostIo(char* base) : c(base) {}
    template <typename T = char> T* in(const void* host, size_t bytes) { return host ? add<T>(host, nullptr, bytes, false) : nullptr; }
    template <typename T = char> T* out(void* host, size_t bytes, bool always = false) { return (host || always) ? add<T>(nullptr, host, bytes, false) : nullptr; }
    template <typename T = char> T* zeroed(void* host, size_t bytes) { return add<T>(nullptr, host, bytes, true); }
    template <typename T> T* add(const void* in, void* out, size_t bytes, bool zero) {
        char* d = c.take<char>(bytes);
        arr[n++] = {d, in, out, bytes, zero};
        return reinterpret_cast<T*>(d);
    }
};

template <class O>
int ensure_ws(O* o, size_t bytes) {
    return bytes <= o->ws_bytes ? SRBDQP_OK : grow(o, o->ws, o->ws_bytes, bytes + bytes / 4, o->stream, "hipMalloc workspace");
}

// a host-buffer call on o's stream: arrays(io) names its arrays (run twice: a dry run for the size, then carved from o's workspace), then upload, clear,
// run(stream) -- the device entry point --, download, synchronise
template <class O, class Arrays, class Run>
int host_call(O* o, Arrays&& arrays, Run&& run) {
    HostIo sz(nullptr);
    arrays(sz);
    int rc = ensure_ws(o, sz.c.off);
    if (rc != SRBDQP_OK) return rc;
    HostIo io(o->ws);
    arrays(io);
    hipStream_t st = o->stream;
    for (int i = 0; i < io.n; ++i) {
        const HostIo::Arr& x = io.arr[i];
        if (x.in) HIP_TRY(o, hipMemcpyAsync(x.dev, x.in, x.bytes, hipMemcpyHostToDevice, st));
        if (x.zero) HIP_TRY(o, hipMemsetAsync(x.dev, 0, x.bytes, st));
    }
    rc = run(st);
    if (rc != SRBDQP_OK) return rc;
    for (int i = 0; i < io.n; ++i) {
        const HostIo::Arr& x = io.arr[i];
        if (x.out) HIP_TRY(o, hipMemcpyAsync(x.out, x.dev, x.bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(o, hipStreamSynchronize(st));
    return SRBDQP_OK;
}

// Iteration at which a solve of this handle re-balances rho (0 = never), and how many times it may (*count).  srbdqp_config.rho_restart_iter: > 0 that
// iteration, < 0 off, 0 = automatic:
//  * N > 10: the long horizons have a 1 - 3 % tail of slow QPs and a set-up that is two thirds of a solve: N = 12: 70 x 2, N = 16: 80 x 3, N = 20: 125 x 1,
//    N = 24: 100 x 2 (below) -- N = 20 single support: 98.4 % solved without, 99.3 % with; N = 20 double support with the (0.7, 4) penalties: 17 % of the QPs run past
//    80 iterations, 8 % past 100, 3 % past 125 -- an earlier restart sends too many through a second set-up: 80 instead of 125 cost configs[2] 10 % for 99.90 %
//    instead of 99.89 % solved;
//  * N <= 10: every 55 iterations, up to twice, each time from the rho of the pass before it -- 99.3 % -> 99.93 % of the configs[1] QPs solved inside the same
//    250-iteration cap, at fewer iterations in total (34.8 -> 33.8).  Measured on the one-wave kernel (configs[1], 4 x 4096 QPs; M QP/s, solved, duration of one
//    isolated launch): off 30.6, 0.9929, 0.19 ms; 80 x 1 30.2, 0.9981, 0.21; 65 x 2 30.0, 0.9991, 0.24; 55 x 2 29.6, 0.9993, 0.24; 70 x 3 29.2, 0.9996, 0.27;
//    50 x 3 29.5, 0.9999.
// Since round 4 the rule is the SAME for every kernel and batch size (round 3: at N <= 10 only where the one-wave kernel ran a call of >= 4096 QPs, so one QP
// could end SOLVED in a large batch and MAX_ITER alone): what differs is how the passes run --
//    one-wave kernel:      in place, inside the kernel (srbdqp_setup1.hpp RST), or handed to the next launch on the stream (SRBDQP_FLAG_DEFER_TAIL);
//    every other kernel:   one more launch over the same grid per pass, in which only the workgroups of the QPs the pass before left at its cap do anything
//                          (the rho of a pass reaches the next one through RestartSet::rho);
//    staged (batch-1) call: the host starts a further pass only when a status[] asks for it (4 % of the calls take a second launch, 1 % a third).
// The price where a call is small: it cannot end before its slowest QP, and a restarted one is a chain of up to three set-ups and 250 iterations (0.22 ms
// against 0.16 ms for 250 iterations at one rho): 512 QPs per call on the one-wave kernel 7.2 -> 5.2 M QP/s.  rho_restart_iter = -1 buys that back.
inline int restart_iter_of(const srbdqp_handle* h, int* count = nullptr) {
    const srbdqp_config& c = h->cfg;
    const int rk = resolve_kernel(c);
    if (count) *count = 1;
    if (rk != SRBDQP_KERNEL_COMPACT && rk != SRBDQP_KERNEL_WRENCH) return 0;   // v0 / v1 have no restart
    int r = c.rho_restart_iter;
    const bool automatic = r == 0;
    // automatic, by horizon (C oracle sweeps, 768 - 1024 QPs per case, round 4; solved share and restart events -- i.e. repeated set-ups -- per QP):
    //   N <= 10  55 x 2;   N = 12  70 x 2 (mixed 99.6 -> 100 %, single 99.3 -> 99.9 %, 0.025 -> 0.05 events);   N = 16  80 x 3 (99.4 -> 100 %, 0.04 -> 0.08);
    //   N = 20  125 x 1 (more re-balancings buy nothing inside the 250-iteration cap);   N = 24  100 x 2 (mixed 98.05 -> 98.96 %, double 99.6 -> 99.7 %,
    //   0.13 -> 0.22 events; 80 x 3 would give 99.6 / 99.9 % for 0.32 events: a set-up is two thirds of a solve there)
    const int N = c.horizon;
    if (automatic) r = (N <= 10) ? 55 : (N == 12 ? 70 : (N == 16 ? 80 : (N == 24 ? 100 : 125)));
    if (count) *count = c.rho_restart_count > 0 ? c.rho_restart_count : (!automatic ? 1 : ((N <= 10 || N == 12) ? 2 : (N == 16 ? 3 : (N == 24 ? 2 : 1))));   // (every other N > 10 -- the live horizons 11, 13 ... -- as N = 20: oracle default_restart)
    // at most three re-balancings, on every kernel (round 5): the one-wave kernel runs its continued passes as three straight copies of the body -- a loop around it
    // costs the whole kernel 30 registers and puts 52 - 72 bytes per lane in scratch memory -- and the rule is the same for every kernel and batch size
    if (count && *count > 3) *count = 3;
    return (r > 0 && r < c.max_iter) ? r : 0;
}

// Batches of at least this many QPs of the small instantiations (<= 64 presolved variables) run with one wave per QP
// (launch_wave); the staged (completion-word) path and the big instantiations use the 4-wave kernel.  Until round 4 the cross-over of the per-call time was 512
// QPs; with the rho restart on at every batch size (in place on the one-wave kernel, one more launch per pass on the 4-wave one) the one-wave kernel is the
// faster one at EVERY size (tools/threshold_probe.py, us per synchronised call, 4-wave / one-wave: B = 1 60 / 55, 32 67 / 61, 128 72 / 64, 256 163 / 149,
// 512 238 / 192, 4096 483 / 289).
constexpr int kSplitMinBatch = 1;

// Batches of at least this many QPs with more than 2 stance contacts in a step go to the general kernel at N <= 10 too
// (measured, tools/schedule_bench.py, 4096 QPs: N = 10 double support 13.5 M QP/s against 4.2 M on the 4-wave compact kernel,
// mixed gait 13.9 M against 6.5 M); smaller ones stay on the 4-wave kernel (lowest latency).
constexpr int kWrenchMinBatch = 512;      // re-measured in round 4 (uniform rho restart; tools/schedule_bench.py, M QP/s 4-wave / general): N = 10 mixed gait 256 QPs 1.72 / 1.63,
                                          // 512 3.10 / 3.28, 768 3.98 / 4.67, 1024 4.63 / 6.06; double support 256 1.70 / 2.45, 512 2.61 / 4.28 (round 2: 768)
constexpr int kTail1MaxBatch = 8;              // staged calls of up to this many QPs on <= 2 stance contacts per step: the 4-wave set-up + one-wave iteration kernel
constexpr int kStagedWrenchMinVars = 60;   // staged call: presolved variables (3 per stance contact) above which the wrench-space kernel's low-latency
                                          // instantiation wins (B = 1, N = 10: mixed gait, 72 variables, 74 us compact / 69 us; double support, 120, 107 / 69)
constexpr int kWrenchMinBatchN20 = 256;   // N = 20: one workgroup per CU on the compact kernel, two on the general one

// fp32 calls of at least this many QPs are split by tile precision (two launches + the classification kernel); smaller
// ones run on fp64 tiles, where the third workgroup per CU would stay empty anyway.
constexpr int kTileClassMinBatch = 512;

// ---- the planner: which kernel a solve of B QPs on this handle runs, and how its rho restart runs.  Every test that picks a kernel is here, and every threshold
// above is read here only; launch() and the launchers execute the Plan, every pass of the call the same one. ----
// maxs: the caller's bound on the stance contacts per step (the config's, the batch's own flags scanned, or 4); neff: the most presolved variables (3 x stance
// contacts) of one QP (the staged call); dump: the assembly dump -- of the general kernel, whatever a solve would run, if `general` (srbdqp_assemble_wrench_f64)
Plan plan_solve(const srbdqp_handle* h, const Call& c, int B, int maxs, int neff = 0, bool dump = false, bool general = false) {
    const srbdqp_config& cfg = h->cfg;
    const int N = cfg.horizon, k = cfg.kernel;
    const bool stamps = h->stamps != nullptr, defer = (cfg.flags & SRBDQP_FLAG_DEFER_TAIL) != 0;
    Plan p;
    // ---- the general kernel (srbdqp_wrench.hpp)?  The compact kernel exists with up to 4 stance contacts per step at N <= 10, with at most 2 at N = 12 - 20
    // (per-QP records, weights and wrenches, contact normals, a live horizon: only the general kernel reads them)
    const unsigned state = state_of(h);                  // (rank-aware steps alone do not ask for the general kernel: the compact kernels have no wrench steps)
    general = general || k == SRBDQP_KERNEL_WRENCH || c.f32 || N == 24 || (state & ~bit(Form::RankAware)) || c.side.kind != Side::None;   // (a staged wrench / normals call: MODE 7 / MODE 4, for every contact pattern)
    // N = 20 single support too, for batches: the general kernel holds 2 workgroups per CU there, the compact one 1
    // (tools/schedule_bench.py, 16,384 QPs: 2.85 M QP/s against 1.95 M; at N = 12 / 16 the compact kernel wins, 7.1 / 4.9 M
    // against 5.7 / 4.2 M)
    if (!general && N > 10) general = maxs > 2 || (N == 20 && k == SRBDQP_KERNEL_AUTO && B >= kWrenchMinBatchN20 && !stamps && !c.staged);
    // N <= 10 with more than 2 stance contacts in a step: batches (the 4-wave kernel wins up to two QPs per CU) AND the staged
    // low-latency path -- the reference's own call feeds full double support on every step (run_simulation.py:100-101), where the
    // wrench-space problem is 60 x 60 against the 120 x 120 dense K of the compact kernel (round 3, tools/latency_patterns.py:
    // B = 1 double support p50 82 us against 112 us)
    // (the low-latency instantiation is one workgroup per CU, tuned and measured at B = 1: the same bound as the compact kernel's TAIL1 path)
    else if (!general && k == SRBDQP_KERNEL_AUTO && maxs > 2 && !stamps)
        general = B >= kWrenchMinBatch || (c.staged && B <= kTail1MaxBatch && N >= 8 && neff > kStagedWrenchMinVars);
    // the staged low-latency instantiations (_lat) of the 4-wave and the general kernel: a call that publishes the completion word, a few QPs
    const bool lat = c.signal && !dump && B <= kTail1MaxBatch && !(cfg.flags & SRBDQP_FLAG_NO_LAT);
    if (general) {           // (p.family as it is)
        const bool side = !dump && !c.f32 && N <= kRobotsMaxHorizon;   // (the side-input forms are fp64 batch kernels for N <= 20, and the dump has none)
        p.form = launch_form(side ? state : state & ~kSideInputs);
        if (p.form == Form::Plain && !c.f32 && N <= 10 && lat) p.form = Form::Lat;
        // a call with a side input of its own (the entry points admit a staged one on a Plain handle only, N <= 20): the low-latency MODE 7 / MODE 4 instantiation
        // where the plain call has one, else the batch one
        const bool lat_side = N <= 10 && lat;
        if (c.side.kind == Side::ExtWrench) p.form = lat_side ? Form::LatExtWrench : Form::ExtWrench;
        else if (c.side.kind == Side::Normals) p.form = lat_side ? Form::LatNormals : Form::Normals;
        p.tile_classes = c.f32 && !c.signal && !(cfg.flags & SRBDQP_FLAG_F64_TILES) && (B >= kTileClassMinBatch || (cfg.flags & SRBDQP_FLAG_F32_TILES));
    } else {
        // ---- the presolved family (srbdqp_compact.hpp): <N, 2> or, at N <= 10, <N, 4>; the one-wave kernel where the QP has at most 64 presolved variables
        // (Setup1Smem::supported) unless a stamp buffer or the completion word needs the 4-wave one (the dump carries neither)
        p.maxs = (N > 10 || maxs <= 2) ? 2 : 4;
        const bool fits_wave = N <= 10 && (N == 4 || maxs <= 2);
        const bool want_wave = k == SRBDQP_KERNEL_WAVE || (k == SRBDQP_KERNEL_AUTO && B >= kSplitMinBatch);
        if (fits_wave && want_wave && (!stamps || dump || k == SRBDQP_KERNEL_WAVE) && !c.signal) p.family = Family::Wave;
        else if (k == SRBDQP_KERNEL_SPLIT && !dump && !stamps && !c.signal) { p.family = Family::Split; p.wave_setup = fits_wave && !(cfg.flags & SRBDQP_FLAG_SETUP4); }
        else { p.family = Family::Compact; if (p.maxs == 2 && lat) p.form = Form::Lat; }
    }
    // ---- the rho restart (periods and counts: restart_iter_of, at most three re-balancings -- what the lists of a set and of a launch stream hold)
    if (dump || stamps || B < 1 || restart_iter_of(h) <= 0) return p;
    // (the staged call starts its further passes itself, and only when a status asks for one: c.lazy)
    if (p.family != Family::Wave) p.restart = (defer && !c.lazy && !c.signal) ? Restart::Deferred : Restart::Launches;
    else if (!defer) p.restart = Restart::InPlace;
    else { p.family = Family::WaveDefer; p.maxs = wave_defer_maxs(N); p.restart = Restart::Deferred; }   // continuations ride in the next launch on this stream (srbdqp_flush() completes them)
    return p;
}

inline bool general_allowed(const srbdqp_config& c) { return c.kernel == SRBDQP_KERNEL_AUTO || c.kernel == SRBDQP_KERNEL_WRENCH; }   // (a side input needs the general kernel: variant_check_batch)
inline int plan_two_phase(int maxs) { return maxs <= 2 ? 2 : 4; }   // the MAXS of the two-phase call (N <= 10): the presolved family's rule, kept from the set-up for phase 2

// a launch stream's restart sets for batches of up to B QPs (nsets = 3: with the lists of the deferred passes); growing waits for this stream and its tail only
int ensure_restart_buffers(srbdqp_handle* h, srbdqp_handle::StreamSlot* slot, hipStream_t st, size_t B, int nsets = 1) {
    const size_t N = (size_t)h->cfg.horizon;
    if (slot->rb.fits(B, B * 20 * N, nsets)) return SRBDQP_OK;
    HIP_TRY(h, hipStreamSynchronize(st));
    if (const int rc = tail_drain(h, slot->rtail)) return rc;
    return carve_restart_sets(h, slot->rb, B, B * 20 * N, nsets, nsets > 1 ? 4 : 0, B <= 64 ? B * 12 * N : 0);   // (ubuf: only the staged path uses it: small batches)
}

// run what the lists of this launch stream still hold: one launch, one workgroup per record the lists can hold, each running every pass its QP has left;
// enqueued on st, no host synchronisation
int flush_slot(srbdqp_handle* h, srbdqp_handle::StreamSlot* slot, hipStream_t st) {
    if (!slot->tail || !slot->tail_live) return SRBDQP_OK;
    int rcount = 1;
    const int restart = restart_iter_of(h, &rcount);
    KArgs a = base_args(h->cfg, 0);
    a.restart_every = restart; a.restart_max = rcount;
    // ONE launch: a flush workgroup runs every pass its QP has left (srbdqp_setup1.hpp, FLUSH)
    if (const int rc = launch_wave_defer_any(h, a, st, slot)) return rc;
    slot->tail_live = false;
    return SRBDQP_OK;
}

// lists for launches of up to B QPs that may re-balance up to rmax times (sized for the share that really continues; a full list is not an error)
int ensure_tail_lists(srbdqp_handle* h, srbdqp_handle::StreamSlot* slot, hipStream_t st, size_t B, int rmax) {
    // Round 5: sized for the share of a launch that really continues, not for every QP of it (rmax + 1) times over (1.2 GB per stream at 65,536 QPs).  About 4 % of a
    // configs[1] batch reach the first mark and 1 % the second; a list holds a QUARTER of the largest launch (at least 8192 records, never more than the
    // (rmax + 1) B that can exist): 16,448 records x 3 lists x 1664 B = 82 MB at 65,536 QPs, 41 MB at 4096.  A QP that finds its list full runs its remaining
    // passes in place (srbdqp_setup1.hpp, srbdqp_wave_defer_kernel): same results, it only holds its own launch up as the restart in place would.
    size_t want = B / 4 > 8192 ? B / 4 : 8192;
    if (want > (size_t)(rmax + 1) * B) want = (size_t)(rmax + 1) * B;
    want += 64;
    if (slot->tail && slot->tail_cap >= want) return SRBDQP_OK;
    if (slot->tail) {                                               // growing: finish what the old lists hold, then let go of them
        int rc = flush_slot(h, slot, st);
        if (rc != SRBDQP_OK) return rc;
        HIP_TRY(h, hipStreamSynchronize(st));
        HIP_TRY(h, hipFree(slot->tail)); slot->tail = nullptr; slot->tail_cap = 0;
    }
    if (!slot->tail_cnt) {
        HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&slot->tail_cnt), 64));
    }
    const size_t cap = want;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&slot->tail), 3 * cap * srbdqp::kTailRecDoubles * sizeof(double));
    if (e != hipSuccess) { h->err = std::string("hipMalloc tail lists: ") + hipGetErrorString(e); return SRBDQP_E_NOMEM; }
    slot->tail_cap = cap;
    slot->tail_k = 0;
    for (auto& v : slot->tail_hist) v = 0;
    HIP_TRY(h, hipMemsetAsync(slot->tail_cnt, 0, 64, st));
    return SRBDQP_OK;
}

// Restart pass p (1 = the first re-balancing) of a solve whose first pass ran with the arguments a1 (status / y_out / resid_out set, max_iter = the restart
// period): the same grid again; the workgroup of a QP that the pass before left at its cap re-balances its rho from the maxima of its last check -- from the rho of
// THAT pass -- and continues from its own (x, y), every other workgroup leaves at once.  No selection kernel and no list between the passes: a one-workgroup kernel
// queued behind a chip-filling launch of another stream waits ~150 us for its turn at the dispatcher (rocprofv3 timeline, round 2), which cost more than the
// pass itself.  last: no further pass may follow (p = rcount, or the cap on the total comes first: oracle solve_with_restart).  rho: the two buffers through
// which the rho of a pass reaches the one behind it.  Every multi-pass solve builds its passes here (run_restart_passes, and the staged call's host-driven loop).
struct Pass { KArgs a; bool last; };
Pass restart_pass(const KArgs& a1, int p, int rcount, int max_iter, double* const rho[2]) {
    const int every = a1.max_iter;
    const int done = p * every;                             // iterations of a QP that every pass so far left at its cap
    const int left = max_iter - done;                       // the cap is on the total
    const bool last = p >= rcount || every >= left;
    KArgs a2 = a1;
    a2.resid_in = a1.resid_out;
    a2.warm_u = a1.u_dev ? a1.u_dev : a1.u_out;             // newtons, as a caller's warm start would be (the device copy of a staged first pass)
    a2.u_dev = (a1.u_dev && !last) ? a1.u_dev : nullptr;    // ... refreshed by every pass another one may follow
    a2.warm_y = a1.y_out;
    a2.max_iter = last ? left : every;
    a2.iters_base = done;
    a2.resid_out = last ? nullptr : a1.resid_out;           // (a workgroup reads its entry when it starts and writes it when it ends)
    a2.rho_qp = (p == 1) ? a1.rho_qp : rho[p % 2];
    a2.rho_out = last ? nullptr : rho[(p + 1) % 2];
    return {a2, last};
}

// The first pass of such a solve with the arguments a: capped at the restart period, its maxima into the set, and the set's y / status where the caller passes none
// (the pass behind it warm-starts from them).
KArgs first_pass_args(const KArgs& a, int restart, const RestartSet& set) {
    KArgs a1 = a;
    a1.max_iter = restart;
    a1.resid_out = set.resid;
    if (!a1.y_out) { a1.y_out = set.ybuf; a1.y_capped_only = 1; }
    if (!a1.status) a1.status = set.stbuf;
    return a1;
}

// ... and the passes behind it, enqueued on st: launch_pass(pass, p, st) adds what is its owner's and launches pass p.  What differs between the owners:
//  * batch, deferred (solve_deferred_passes): the list of QPs the pass before left at its cap is the dispatch order -- working workgroups first;
//  * ragged (ragged_device_impl): the bucket's whole grid again through launch_wrench on the bucket's handle -- perm holds the bucket's members there;
//  * batch, in the caller's stream (solve_device_impl): the whole grid again, the completion word on the last pass;
//  * the staged call is host-driven (srbdqp_solve_staged_f64): its first pass writes u_dev, and a pass follows only when a status asks for it -- its own loop.
template <class LaunchPass>
int run_restart_passes(const KArgs& a1, int rcount, int max_iter, const RestartSet& set, hipStream_t st, LaunchPass&& launch_pass) {
    for (int p = 1; p <= rcount; ++p) {
        Pass pass = restart_pass(a1, p, rcount, max_iter, set.rho);
        const int rc = launch_pass(pass, p, st);
        if (rc != SRBDQP_OK || pass.last) return rc;
    }
    return SRBDQP_OK;
}

// the launch publishes the completion word with the handle's current sequence number
void signal_args(const srbdqp_handle* h, KArgs& a) { a.done_flag = h->done_dev; a.done_count = h->done_count; a.done_value = h->done_seq; }
int32_t next_seq(srbdqp_handle* h) { return h->done_seq = (h->done_seq == INT32_MAX) ? 1 : h->done_seq + 1; }

// SRBDQP_FLAG_DEFER_TAIL on a kernel that restarts by further launches: the first pass on the caller's stream, the restart passes on the slot's own tail stream
// behind an event -- beside whatever the caller enqueues next, e.g. the next batch's first pass -- each taking the list of QPs the pass before it left at its cap
// as its dispatch order (working workgroups first; the rest of the grid leaves after one scalar load).  Outputs of the continued QPs arrive when the tail
// stream gets there; srbdqp_flush() makes the caller's stream wait for it.
int solve_deferred_passes(srbdqp_handle* h, const Call& c, const KArgs& a, hipStream_t lst, int restart, int rcount) {
    auto* slot = stream_slot(h, lst);
    if (!slot) return SRBDQP_E_INVALID;
    if (const int rc = ensure_restart_buffers(h, slot, lst, (size_t)a.B, kRestartSets)) return rc;
    Tail& tail = slot->rtail;
    if (!tail.st) {
        if (const int rc = tail_create(h, tail)) return rc;
        HIP_TRY(h, hipEventCreateWithFlags(&slot->ev_main, hipEventDisableTiming));
    }
    const int k = next_set(slot->rs_k, kRestartSets);
    const RestartSet& set = slot->rb.set[k];
    if (const int rc = tail_wait(h, tail, k, lst)) return rc;   // the set's last user (three solves ago) has finished its passes
    HIP_TRY(h, hipMemsetAsync(set.cnt, 0, 16 * sizeof(int32_t), lst));
    KArgs a1 = first_pass_args(a, restart, set);
    a1.cap_list = set.list[0]; a1.cap_count = set.cnt;
    if (const int rc = launch(h, c, a1, lst, 1)) return rc;
    HIP_TRY(h, hipEventRecord(slot->ev_main, lst));
    HIP_TRY(h, hipStreamWaitEvent(tail.st, slot->ev_main, 0));
    const int rc = run_restart_passes(a1, rcount, h->cfg.max_iter, set, tail.st, [&](Pass& pass, int p, hipStream_t st) {
        pass.a.perm = set.list[p - 1]; pass.a.count_ptr = set.cnt + (p - 1);
        pass.a.cap_list = pass.last ? nullptr : set.list[p]; pass.a.cap_count = pass.last ? nullptr : set.cnt + p;
        return launch(h, c, pass.a, st, 2);
    });
    return rc != SRBDQP_OK ? rc : tail_close(h, tail, k);
}

// common body of the device-buffer entry points; the element type of the caller's buffers is c.f32 ? float : double
int solve_device_impl(srbdqp_handle* h, const Call& c, int32_t B, const void* x0, const void* x_ref, const void* foot, const uint8_t* contact,
                      const void* pcom, const void* warm_u, const void* warm_y, void* u_out, void* x_out, void* y_out,
                      int32_t* status, int32_t* iters, void* stream) {
    if (B < 0 || (B > 0 && (!x0 || !x_ref || !foot || !contact || !u_out))) { h->err = "null input/output pointer"; return SRBDQP_E_INVALID; }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!c.staged) if (const int rq = aql_quiesce(h)) return rq;
    KArgs a = base_args(h->cfg, B, x0, x_ref, foot, contact, pcom);
    a.warm_u = static_cast<const double*>(warm_u); a.warm_y = static_cast<const double*>(warm_y);
    a.u_out = static_cast<double*>(u_out); a.x_out = static_cast<double*>(x_out); a.y_out = static_cast<double*>(y_out);
    a.status = status; a.iters = iters;
    a.stamps = h->stamps;
    if (c.signal) signal_args(h, a);
    hipStream_t lst = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
    if (c.use_hint && h->sched_hint && B > 1 && (size_t)B <= h->sched_hint_len) {
        auto* slot = stream_slot(h, lst);
        if (!slot) return SRBDQP_E_INVALID;
        const int rc = grow(h, slot->perm, slot->perm_cap, (size_t)B, lst, "hipMalloc dispatch order");   // (a previous launch on this stream may still read the old order)
        if (rc != SRBDQP_OK) return rc;
        hipLaunchKernelGGL(srbdqp_schedule_kernel, dim3(1), dim3(1024), 0, lst, h->sched_hint, slot->perm, (int)B);
        a.perm = slot->perm;
    }
    const Plan& p = c.plan;
    int rcount = 1;
    const int restart = p.restart == Restart::Off ? 0 : restart_iter_of(h, &rcount);
    if (p.restart == Restart::InPlace || p.family == Family::WaveDefer) { a.restart_every = restart; a.restart_max = rcount; }   // the one-wave kernel restarts in place
    if (p.family == Family::WaveDefer) {   // ... or not at all: continuations deferred to the next launch on this stream (srbdqp_flush() completes them)
        auto* slot = stream_slot(h, lst);
        if (!slot) return SRBDQP_E_INVALID;
        if (const int rc = ensure_tail_lists(h, slot, lst, (size_t)B, rcount)) return rc;
        return launch_wave_defer_any(h, a, lst, slot);
    }
    if (p.restart == Restart::Off || p.restart == Restart::InPlace) return launch(h, c, a, lst);
    if (p.restart == Restart::Deferred) return solve_deferred_passes(h, c, a, lst, restart, rcount);

    // ---- several passes: cap the first at rho_restart_iter, re-balance rho for the QPs that reach it, continue those (up to rcount times)
    auto* slot = stream_slot(h, lst);
    if (!slot) return SRBDQP_E_INVALID;
    if (const int rc = ensure_restart_buffers(h, slot, lst, (size_t)B)) return rc;
    // in the caller's stream: set 0 -- on a handle with SRBDQP_FLAG_DEFER_TAIL (a staged or completion-word solve comes through here) behind the passes of the
    // deferred solve that used it last, as that path does: it must not overwrite what a tail pass still reads
    const RestartSet& set = slot->rb.set[0];
    if (const int rc = tail_wait(h, slot->rtail, 0, lst)) return rc;
    KArgs a1 = first_pass_args(a, restart, set);
    if (!c.lazy) { a1.done_flag = nullptr; a1.done_count = nullptr; }
    if (c.lazy && slot->rb.ubuf && !c.f32) a1.u_dev = slot->rb.ubuf;   // (the staged arrays are host memory: the pass behind this one reads its warm start on the device)
    const int rc = launch(h, c, a1, lst, c.lazy ? 0 : 1);
    if (c.lazy) { c.lazy->a1 = a1; c.lazy->rcount = rcount; c.lazy->set = &set; c.lazy->pending = (rc == SRBDQP_OK); }   // (staged path: the host looks at status[] before a second pass)
    if (rc != SRBDQP_OK || c.lazy) return rc;
    return run_restart_passes(a1, rcount, h->cfg.max_iter, set, lst, [&](Pass& pass, int, hipStream_t st) {
        if (pass.last && a.done_flag) signal_args(h, pass.a);
        return launch(h, c, pass.a, st, 2);
    });
}

// ---- the per-QP side inputs: robot records, cost weights, contact normals ----
// To the host each is one thing: an optional per-QP device array (PerQp) that the general kernel reads and every other call refuses, owned by the library (host
// setter) or borrowed (_device setter).  One descriptor per kind says what differs; the setters themselves exist once ("the setters of the per-QP side inputs"
// below).  A further side input is one more descriptor, one more member and its extern "C" lines.
static_assert(sizeof(srbdqp_robot) == 64 && offsetof(srbdqp_robot, inertia) == 8 && offsetof(srbdqp_robot, mu) == 32 &&
              offsetof(srbdqp_robot, fz_min) == 40 && offsetof(srbdqp_robot, fz_max) == 48 && offsetof(srbdqp_robot, reserved) == 56,
              "the kernels read a record as 8 doubles (srbdqp_wrench.hpp qp_robot)");
static_assert(sizeof(srbdqp_weights) == 128 && offsetof(srbdqp_weights, r_diag) == 104 && offsetof(srbdqp_weights, reserved) == 112,
              "the kernels read a record as 16 doubles (srbdqp_wrench.hpp qp_weights_to_lds)");

// the rules of include/srbdqp.h (the same ones the kernel applies to device records, srbdqp_wrench.hpp qp_robot); null = valid, else what is wrong
const char* robot_fault(const srbdqp_robot& r) {
    auto fin = [](double v) { return std::isfinite(v); };
    if (!fin(r.mass) || !(r.mass > 0.0)) return "mass must be finite and > 0";
    for (int i = 0; i < 3; ++i) if (!fin(r.inertia[i]) || !(r.inertia[i] > 0.0)) return "inertia must be finite and > 0";
    if (!fin(r.mu) || !(r.mu > 0.0)) return "mu must be finite and > 0";
    if (!fin(r.fz_min) || !fin(r.fz_max) || !(r.fz_min >= 0.0) || !(r.fz_min <= r.fz_max)) return "need finite 0 <= fz_min <= fz_max";
    if (r.reserved != 0.0) return "reserved must be 0";
    return nullptr;
}

// the rules of include/srbdqp.h (the same ones the kernel applies to device records, srbdqp_wrench.hpp qp_weights_to_lds); null = valid, else what is wrong
// ("finite" is < SRBDQP_WEIGHT_MAX = 1e300 on both sides: the kernel tests one bound, and r_diag s s must not overflow)
const char* weights_fault(const srbdqp_weights& r) {
    for (int i = 0; i < SRBDQP_NX; ++i) if (!(r.q_diag[i] >= 0.0 && r.q_diag[i] < SRBDQP_WEIGHT_MAX)) return "q_diag must be finite (< 1e300) and >= 0";
    if (!(r.r_diag > 0.0 && r.r_diag < SRBDQP_WEIGHT_MAX)) return "r_diag must be finite (< 1e300) and > 0";
    if (r.reserved[0] != 0.0 || r.reserved[1] != 0.0) return "reserved must be 0";
    return nullptr;
}

// the rules of include/srbdqp.h (the same ones the kernel applies to a device array, srbdqp_wrench.hpp contact_frame_to_lds); null = valid, else what is wrong
const char* normal_fault(const double* n) {
    if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2])) return "every entry must be finite";
    const double nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(nn >= 0.5 && nn <= 2.0)) return "need 0.5 <= |n| <= 2";
    if (!(n[2] * (1.0 / nn) >= 0.5)) return "need n_z >= 0.5 |n| (slopes to 60 degrees)";
    return nullptr;
}

// the rule of include/srbdqp.h for one value of an external wrench (the same one the kernel applies to a device array, srbdqp_wrench.hpp
// qp_ext_wrench_to_lds: one bound, SRBDQP_EXT_WRENCH_MAX, on both sides; NaN fails it); null = valid, else what is wrong
const char* ext_wrench_fault(const double* v) {
    return std::fabs(*v) <= SRBDQP_EXT_WRENCH_MAX ? nullptr : "every value must be finite with |value| <= 1e6";
}

// A descriptor: the owner's member (of), the element type T, the per-element test (fault), the handle check (form: its row of kFormRows; n24: the N = 24 text), the
// hipMalloc label (alloc), and the words of the messages (name: srbdqp_set_<name>, srbdqp_ragged_set_<name>; what, which " on a ragged object" follows; count
// and unit: the "B > length" messages).  RecordIn has what a kind of one record per QP need not say again: the elements per QP (per_qp), the elements one
// fault test covers (stride), how a message locates element group i (where).  The two kinds a staged call can carry (ExtWrenchIn, NormalsIn) also say which
// Side they are, where the handle keeps their staging array (staged), the value a fresh one holds (neutral), and the words in which the staged texts differ
// (staged_label: of the hipHostGetDevicePointer message; verb: "<noun> is / are read by the general kernel only"; staged_n24).
struct RecordIn {
    static constexpr const char* unit = "record";
    static constexpr size_t stride = 1;
    template <class O> static size_t per_qp(const O*) { return 1; }
    template <class O> static std::string where(const O*, size_t i) { return "record " + std::to_string(i); }
};

struct RobotsIn : RecordIn {
    using T = srbdqp_robot;
    static constexpr const char* name = "robots";
    static constexpr const char* what = "per-QP robot records";
    static constexpr const char* alloc = "hipMalloc robot records";
    static constexpr Form form = Form::Robots;
    template <class O> static PerQp<T>& of(O* o) { return o->robots; }
    static const char* fault(const T* e) { return robot_fault(*e); }
    static std::string count(size_t len) { return std::to_string(len) + " robot records"; }
    static std::string n24(const char*) { return "per-QP robot records: not at N = 24 (no instantiation of the general kernel reads them there without scratch memory, DESIGN.md section 11)"; }
};

struct WeightsIn : RecordIn {
    using T = srbdqp_weights;
    static constexpr const char* name = "weights";
    static constexpr const char* what = "per-QP cost weights";
    static constexpr const char* alloc = "hipMalloc weight records";
    static constexpr Form form = Form::Weights;
    template <class O> static PerQp<T>& of(O* o) { return o->weights; }
    static const char* fault(const T* e) { return weights_fault(*e); }
    static std::string count(size_t len) { return std::to_string(len) + " weight records"; }
    static std::string n24(const char*) { return "per-QP cost weights: not at N = 24 (no instantiation of the general kernel reads them there without scratch memory, DESIGN.md section 15)"; }
};

struct NormalsIn {
    using T = double;                                   // a QP has 4 N normals of 3 doubles: [len][N][12]
    static constexpr const char* name = "contact_normals";
    static constexpr const char* what = "contact normals";
    static constexpr const char* alloc = "hipMalloc contact normals";
    static constexpr const char* unit = "block";
    static constexpr Form form = Form::Normals;
    static constexpr size_t stride = 3;
    static PerQp<T>& of(srbdqp_handle* h) { return h->normals; }
    static size_t per_qp(const srbdqp_handle* h) { return 12 * (size_t)h->cfg.horizon; }
    static const char* fault(const T* e) { return normal_fault(e); }
    static std::string where(const srbdqp_handle* h, size_t i) {
        const size_t N = (size_t)h->cfg.horizon;
        return "the normal of (qp " + std::to_string(i / (4 * N)) + ", step " + std::to_string((i / 4) % N) + ", contact " + std::to_string(i % 4) + ")";
    }
    static std::string count(size_t len) { return "contact normals for " + std::to_string(len); }
    static std::string n24(const char* fn) { return std::string(fn) + ": contact normals: not at N = 24 (no instantiation of the general kernel reads them there, DESIGN.md section 13)"; }
    // as the side input of a staged call
    static constexpr Side side = Side::Normals;
    static constexpr const char* staged_label = "staged normals";
    static constexpr const char* verb = "are";
    static srbdqp_handle::StagedSide& staged(srbdqp_handle* h) { return h->staged_normals; }
    static double neutral(size_t i) { return i % 3 == 2 ? 1.0 : 0.0; }               // every normal (0, 0, 1): zeros would break the rule 0.5 <= |n|
    static std::string staged_n24(const char* fn) { return n24(fn); }                // (the text carries the call's name itself)
};

struct ExtWrenchIn {
    using T = double;                                   // 6 doubles per horizon row: a handle takes [len][N][6], a ragged object [rows][6]
    static constexpr const char* name = "external_wrench";
    static constexpr const char* what = "external wrenches";
    static constexpr const char* alloc = "hipMalloc external wrench";
    static constexpr const char* unit = "block";
    static constexpr Form form = Form::ExtWrench;
    static constexpr size_t stride = 1;
    template <class O> static PerQp<T>& of(O* o) { return o->ext; }
    static size_t per_qp(const srbdqp_handle* h) { return 6 * (size_t)h->cfg.horizon; }
    static size_t per_qp(const srbdqp_ragged*) { return 6; }                          // (per row)
    static const char* fault(const T* e) { return ext_wrench_fault(e); }
    static std::string where(const srbdqp_handle* h, size_t i) {
        const size_t N = (size_t)h->cfg.horizon;
        return "the wrench at (qp " + std::to_string(i / (6 * N)) + ", step " + std::to_string((i / 6) % N) + ", component " + std::to_string(i % 6) + ")";
    }
    static std::string where(const srbdqp_ragged*, size_t i) { return "the wrench at (row " + std::to_string(i / 6) + ", component " + std::to_string(i % 6) + ")"; }
    static std::string count(size_t len) { return "an external wrench for " + std::to_string(len); }
    static std::string n24(const char*) { return "an external wrench: not at N = 24 (no instantiation of the general kernel reads it there, DESIGN.md section 16)"; }
    // as the side input of a staged call
    static constexpr Side side = Side::ExtWrench;
    static constexpr const char* staged_label = "staged wrench";
    static constexpr const char* verb = "is";
    static srbdqp_handle::StagedSide& staged(srbdqp_handle* h) { return h->staged_ext; }
    static double neutral(size_t) { return 0.0; }
    static std::string staged_n24(const char* fn) { return std::string(fn) + ": " + n24(fn); }
};

// no side input: what the plain staged calls are instantiated with
struct NoSideIn {
    static constexpr Side side = Side::None;
};

// may this handle take side input K?  (a live horizon, rank-aware steps, another side input it does not combine with: a combined mode would be another copy of
// every instantiation)
template <class K>
int check_handle(srbdqp_handle* h, const char* fn) {
    if (const int rc = require_form(h, fn, forms_of_setter(K::form))) return rc;
    if (h->cfg.horizon > row(K::form).max_horizon) { h->err = K::n24(fn); return SRBDQP_E_INVALID; }
    if (K::form == Form::Normals && (state_of(h) & bit(Form::Robots))) { h->err = std::string(fn) + kNormalsOnRobots; return SRBDQP_E_INVALID; }
    return SRBDQP_OK;
}

// a host array of side input K for `length` QPs: every element by the rules of include/srbdqp.h (then: what the refusal leaves as it was)
template <class K, class O>
int validate(O* o, const typename K::T* host, int32_t length, const char* fn, const char* then = "the previous setting is kept") {
    const size_t groups = (size_t)length * K::per_qp(o) / K::stride;
    for (size_t i = 0; i < groups; ++i)
        if (const char* why = K::fault(host + K::stride * i)) {
            o->err = std::string(fn) + ": " + K::where(o, i) + " is invalid (" + why + "); " + then;
            return SRBDQP_E_INVALID;
        }
    return SRBDQP_OK;
}

// a call over B QPs while side input K is set for fewer: lead + "<B>" + mid + "<K's count> set", then the setter's name (by_setter) and what every QP needs
// (needs), as each owner's wording has them.  A pointer and a length test on the way of a solve; a string only when the refusal fires.
template <class K, class O>
int covers(O* o, long long B, const char* lead, const char* mid, bool by_setter, bool needs) {
    const auto& s = K::of(o);
    if (!s.dev || (size_t)B <= s.len) return SRBDQP_OK;
    o->err = lead + std::to_string(B) + mid + K::count(s.len) + " set";
    if (by_setter) o->err += std::string(" (srbdqp_set_") + K::name + ")";
    if (needs) o->err += std::string(": every QP needs its ") + K::unit;
    return SRBDQP_E_INVALID;
}
template <class K> int covers_batch(srbdqp_handle* h, int32_t B) { return covers<K>(h, B, "solve of ", " QPs with ", true, true); }

// before the library's own copy of a side input is replaced: every solve that may still read it has completed (srbdqp_synchronize, then every other launch
// stream of the handle and its tail streams -- deferred restart passes read them too)
int quiesce_all_streams(srbdqp_handle* h) {
    int rc = srbdqp_synchronize(h);
    if (rc != SRBDQP_OK) return rc;
    rc = srbdqp_flush(h, nullptr);
    if (rc != SRBDQP_OK) return rc;
    for (auto& sl : h->slots) {
        if (!sl.used) continue;
        HIP_TRY(h, hipStreamSynchronize(sl.st));
        if (sl.rtail.st) HIP_TRY(h, hipStreamSynchronize(sl.rtail.st));
    }
    return SRBDQP_OK;
}

// fp64 batch solve of B QPs with a side input set: the general kernel, and a record / a block of normals for every QP
int variant_check_batch(srbdqp_handle* h, int32_t B) {
    const unsigned side = state_of(h) & kSideInputs;
    if (!side) return SRBDQP_OK;
    if (!general_allowed(h->cfg)) {
        h->err = std::string(row(refusal_form(side)).noun) + " are read by the general kernel only: srbdqp_config.kernel must be SRBDQP_KERNEL_AUTO or SRBDQP_KERNEL_WRENCH while they are set";
        return SRBDQP_E_INVALID;
    }
    if (const int rc = covers_batch<WeightsIn>(h, B)) return rc;      // (weights alone, or beside robot records: each length on its own)
    if (const int rc = covers_batch<RobotsIn>(h, B)) return rc;
    if (const int rc = covers_batch<ExtWrenchIn>(h, B)) return rc;
    return covers_batch<NormalsIn>(h, B);
}

}  // namespace

extern "C" {

const char* srbdqp_version(void) { return "srbdqp 0.1 (gfx950, fp64)"; }

int srbdqp_default_config(srbdqp_config* c) {
    if (!c) return SRBDQP_E_INVALID;
    // the caller says how large ITS struct is: a binding built against an older header (a shorter struct) is refused here instead of
    // being written past its end
    if (c->struct_size != (int32_t)sizeof(srbdqp_config)) { g_create_err = "srbdqp_default_config: set cfg->struct_size = sizeof(srbdqp_config) before the call (ABI check)"; return SRBDQP_E_INVALID; }
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(srbdqp_config);
    c->horizon = 10;
    c->device = 0;
    c->flags = 0;
    c->kernel = SRBDQP_KERNEL_AUTO;
    c->max_iter = 250;
    c->check_every = 5;
    c->dt = 0.04;
    c->mass = 34.13385728;
    c->inertia[0] = 8.20564e-2; c->inertia[1] = 8.05015e-2; c->inertia[2] = 0.32353e-2;
    c->mu = 0.8;
    c->fz_min = 10.0; c->fz_max = 1000.0;
    const double q[13] = {300.0, 300.0, 150.0, 400.0, 400.0, 600.0, 1.0, 1.0, 1.0, 20.0, 20.0, 20.0, 0.0};
    for (int i = 0; i < 13; ++i) c->q_diag[i] = q[i];
    c->r_diag = 1.0e-4;
    c->force_scale = 100.0;
    c->rho = 0.0; c->rho_eq_scale = 1.0e3; c->sigma = 1.0e-6; c->alpha = 1.6;
    c->eps_abs = 1.0e-6; c->eps_rel = 1.0e-6;
    c->rho_restart_iter = 0; c->rho_restart_count = 0;
    c->rho_fz_scale = 0.0;
    return SRBDQP_OK;
}

int srbdqp_create(const srbdqp_config* cfg, srbdqp_handle** out) {
    if (!cfg || !out) { g_create_err = "null argument"; return SRBDQP_E_INVALID; }
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(srbdqp_config)) { g_create_err = "srbdqp_config.struct_size mismatch"; return SRBDQP_E_INVALID; }
    const bool live = !horizon_supported(cfg->horizon) && (cfg->flags & SRBDQP_FLAG_ANY_HORIZON) && cfg->horizon >= 1 && cfg->horizon <= SRBDQP_MAX_HORIZON;
    if (!horizon_supported(cfg->horizon) && !live) {
        g_create_err = "unsupported horizon (N in {4, 8, 10, 12, 16, 20, 24}; with SRBDQP_FLAG_ANY_HORIZON every N from 1 to 24)";
        return SRBDQP_E_INVALID;
    }
    if (live && !general_allowed(*cfg)) {
        g_create_err = "SRBDQP_FLAG_ANY_HORIZON: a horizon outside {4, 8, 10, 12, 16, 20, 24} runs on the general kernel only (srbdqp_config.kernel = SRBDQP_KERNEL_AUTO or SRBDQP_KERNEL_WRENCH)";
        return SRBDQP_E_INVALID;
    }
    if ((cfg->flags & SRBDQP_FLAG_RANK_AWARE) && (live || cfg->horizon > row(Form::RankAware).max_horizon)) {
        g_create_err = live ? "SRBDQP_FLAG_RANK_AWARE: not at a live horizon of SRBDQP_FLAG_ANY_HORIZON (the rank-aware instantiations are built for N in {4, 8, 10, 12, 16, 20})"
                            : "SRBDQP_FLAG_RANK_AWARE: not at N = 24 (no instantiation of the general kernel without scratch memory there; N in {4, 8, 10, 12, 16, 20})";
        return SRBDQP_E_INVALID;
    }
    if (cfg->kernel != SRBDQP_KERNEL_AUTO && cfg->kernel != SRBDQP_KERNEL_COMPACT && cfg->kernel != SRBDQP_KERNEL_SPLIT &&
        cfg->kernel != SRBDQP_KERNEL_WAVE && cfg->kernel != SRBDQP_KERNEL_WRENCH) { g_create_err = "unknown srbdqp_config.kernel (the round-1 baselines v0 / v1 are retired)"; return SRBDQP_E_INVALID; }
    if (!(cfg->dt > 0) || !(cfg->mass > 0) || !(cfg->force_scale > 0) || !(cfg->rho >= 0) || !(cfg->sigma > 0) ||
        cfg->max_iter < 1 || cfg->check_every < 1 || !(cfg->mu >= 0) || cfg->max_contacts_per_step < 0 || cfg->max_contacts_per_step > 4) { g_create_err = "invalid constants"; return SRBDQP_E_INVALID; }
    for (int i = 0; i < 13; ++i) if (!(cfg->q_diag[i] >= 0)) { g_create_err = "negative q_diag"; return SRBDQP_E_INVALID; }
    for (int i = 0; i < 3; ++i) if (!(cfg->inertia[i] > 0)) { g_create_err = "inertia must be positive"; return SRBDQP_E_INVALID; }
    if (!(cfg->alpha > 0 && cfg->alpha < 2) || !(cfg->eps_abs >= 0) || !(cfg->eps_rel >= 0) || !(cfg->eps_abs + cfg->eps_rel > 0) ||
        !(cfg->fz_min >= 0) || !(cfg->fz_min <= cfg->fz_max) || !(cfg->r_diag >= 0) || !(cfg->rho_eq_scale > 0) || !(cfg->rho_fz_scale >= 0)) {
        g_create_err = "invalid constants (alpha in (0, 2), eps >= 0, 0 <= fz_min <= fz_max, r_diag >= 0)"; return SRBDQP_E_INVALID;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        g_create_err = "no usable HIP device (this engine has no CPU fallback)";
        return SRBDQP_E_NO_DEVICE;
    }
    srbdqp_handle* h = new (std::nothrow) srbdqp_handle();
    if (!h) { g_create_err = "out of host memory"; return SRBDQP_E_NOMEM; }
    h->cfg = *cfg;
    if (live) {
        h->live_nstar = horizon_above(cfg->horizon, Horizons{});
        h->live_name = "wrench_f64_n" + std::to_string(h->live_nstar) + row(Form::Live).suffix + std::to_string(cfg->horizon);
        // the staged calls run the batch instantiation through the HIP launch, as SRBDQP_FLAG_NO_LAT does (no _lat / *_in kernel reads a live horizon): no AQL queue
        h->aql_tried = true;
        h->aql_why = "SRBDQP_FLAG_ANY_HORIZON: a live horizon runs the batch instantiation of the general kernel";
    }
    if (cfg->flags & SRBDQP_FLAG_RANK_AWARE) {
        // the staged calls of such a handle go through the HIP launch: on the general kernel they run the batch instantiation _ra (no _lat / *_in kernel has rank-aware steps)
        h->aql_tried = true;
        h->aql_why = "SRBDQP_FLAG_RANK_AWARE: the staged calls run the batch instantiation of the general kernel";
    }
    if (h->cfg.rho == 0.0) h->cfg.rho = 0.7;                    // auto (oracle auto_rho()): friction rows
    if (h->cfg.rho_fz_scale == 0.0) h->cfg.rho_fz_scale = 4.0;   // auto (oracle auto_rho_fz_scale()): normal-force rows at 4 rho
    auto fail = [&](const char* what, hipError_t er) {
        g_create_err = std::string(what) + ": " + hipGetErrorString(er);
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        if (h->stage_host) (void)hipHostFree(h->stage_host);
        if (h->done_count) (void)hipFree(h->done_count);
        delete h;
        return SRBDQP_E_HIP;
    };
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipEventCreate(&h->ev0)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipEventCreate(&h->ev1)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipEventCreate(&h->ev_mid)) != hipSuccess) return fail("hipEventCreate", e);
    {   // staging slab for the low-latency path
        const size_t N = (size_t)cfg->horizon, n = 12 * N, m = 20 * N, cap = 16;
        auto carve = [&](char* base, srbdqp_stage& st) {
            Carver c(base);
            st.capacity = (int32_t)cap;
            st.x0 = c.take<double>(cap * 13); st.x_ref = c.take<double>(cap * N * 13); st.foot = c.take<double>(cap * N * 12);
            st.contact = c.take<uint8_t>(cap * N * 4); st.pcom = c.take<double>(cap * N * 3);
            st.warm_u = c.take<double>(cap * n); st.warm_y = c.take<double>(cap * m);
            st.u = c.take<double>(cap * n); st.x = c.take<double>(cap * (N + 1) * 13); st.y = c.take<double>(cap * m);
            st.status = c.take<int32_t>(cap); st.iters = c.take<int32_t>(cap);
            return c.off;
        };
        srbdqp_stage tmp{};
        const size_t body = (carve(reinterpret_cast<char*>(4096), tmp) + 255) & ~size_t(255);   // dry run for the size
        const size_t bytes = body + 256;
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&h->stage_host), bytes, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return fail("hipHostMalloc(staging)", e);
        if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->stage_dev), h->stage_host, 0)) != hipSuccess) return fail("hipHostGetDevicePointer", e);
        std::memset(h->stage_host, 0, bytes);
        carve(h->stage_host, h->stage_h);
        carve(h->stage_dev, h->stage_d);
        h->done_host = reinterpret_cast<volatile int32_t*>(h->stage_host + body);
        h->done_dev = reinterpret_cast<int32_t*>(h->stage_dev + body);
        if ((e = hipMalloc(reinterpret_cast<void**>(&h->done_count), 64)) != hipSuccess) return fail("hipMalloc(done counter)", e);
        if ((e = hipMemset(h->done_count, 0, 64)) != hipSuccess) return fail("hipMemset(done counter)", e);
    }
    *out = h;
    return SRBDQP_OK;
}

int srbdqp_destroy(srbdqp_handle* h) {
    if (!h) return SRBDQP_OK;
    (void)hipSetDevice(h->cfg.device);
    delete h->aql;                                 // (waits for its last kernel)
    h->aql = nullptr;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ws) (void)hipFree(h->ws);
    for (auto& sl : h->slots) {
        tail_destroy(sl.rtail);                          // (waits for its last pass: before the sets go)
        if (sl.perm) (void)hipFree(sl.perm); if (sl.ws) (void)hipFree(sl.ws); if (sl.rb.mem) (void)hipFree(sl.rb.mem);
        if (sl.tail) (void)hipFree(sl.tail); if (sl.tail_cnt) (void)hipFree(sl.tail_cnt);
        if (sl.ev_main) (void)hipEventDestroy(sl.ev_main);
    }
    if (h->done_count) (void)hipFree(h->done_count);
    h->robots.release(); h->weights.release(); h->normals.release(); h->ext.release();
    if (h->fleet.mem) (void)hipFree(h->fleet.mem);
    if (h->terrain.own) (void)hipFree(h->terrain.own);
    if (h->stage_host) (void)hipHostFree(h->stage_host);
    for (const auto& ss : {h->staged_ext, h->staged_normals}) if (ss.host) (void)hipHostFree(ss.host);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SRBDQP_OK;
}

const char* srbdqp_last_error(const srbdqp_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

const char* srbdqp_kernel_name(const srbdqp_handle* h) { return h ? h->kname : "none"; }

const char* srbdqp_batch1_launch_path(const srbdqp_handle* h) {
    if (!h || !h->aql_tried) return "undecided";
    if (h->aql) return "aql";
    static thread_local std::string s;
    s = "hip: " + h->aql_why;
    return s.c_str();
}

int srbdqp_stage_ptrs(srbdqp_handle* h, srbdqp_stage* out) {
    if (!h || !out) return SRBDQP_E_INVALID;
    *out = h->stage_h;
    return SRBDQP_OK;
}

}  // extern "C"

namespace {
// the staged solve of B QPs over the staging arrays, behind its entry point's checks; side: QP b under block b of that staged array, in every pass (or none)
int solve_staged_impl(srbdqp_handle* h, int32_t B, int32_t use_pcom, int32_t use_warm, int32_t want_x, int32_t want_y, const CallSide& side) {
    {   // (the kernel of the call before this one published its completion word before it ended)
        const int rq = aql_quiesce(h);
        if (rq != SRBDQP_OK) return rq;
    }
    const srbdqp_stage& d = h->stage_d;
    h->done_cs = false;            // (set again by a launch that publishes a checksum)
    Lazy lazy;
    Call c;                        // same per-batch kernel choice as the host-buffer API, from the staged contact flags
    const Contacts k = scan_contacts(h->stage_h.contact, (size_t)B, (size_t)h->cfg.horizon, true);
    c.staged = true; c.lazy = &lazy;   // (lazy: the rho restart costs two more launches: only when needed)
    c.side = side;                 // (the restart passes below launch with this Call: they carry the side input)
    // completion: the kernel publishes a sequence number in host memory after its outputs (signal_done()); spinning on it skips the stream's completion
    // interrupt (~15 us)
    c.signal = !(h->cfg.flags & SRBDQP_FLAG_NO_SPIN);
    if (c.signal) next_seq(h);
    c.plan = plan_solve(h, c, B, maxs_or(h->cfg, k.maxs()), k.neff);
    int rc = solve_device_impl(h, c, B, d.x0, d.x_ref, d.foot, d.contact, use_pcom ? d.pcom : nullptr, use_warm ? d.warm_u : nullptr,
                               use_warm ? d.warm_y : nullptr, d.u, want_x ? d.x : nullptr, want_y ? d.y : nullptr, d.status, d.iters, h->stream);
    if (rc != SRBDQP_OK) return rc;
    rc = wait_done(h, c.signal);
    if (rc != SRBDQP_OK || !lazy.pending) return rc;
    for (int p = 1; p <= lazy.rcount; ++p) {                // the first pass of a multi-pass solve ran: a further pass only when a status asks for it
        bool capped = false;
        for (int32_t q = 0; q < B; ++q) capped |= (h->stage_h.status[q] == SRBDQP_MAX_ITER);
        if (!capped) break;
        Pass pass = restart_pass(lazy.a1, p, lazy.rcount, h->cfg.max_iter, lazy.set->rho);
        if (c.signal) { next_seq(h); signal_args(h, pass.a); }
        rc = launch(h, c, pass.a, h->stream, 2);            // (with the first pass's Call: the same plan)
        if (rc != SRBDQP_OK) return rc;
        rc = wait_done(h, c.signal);
        if (rc != SRBDQP_OK || pass.last) break;
    }
    return rc;
}

// ---- the side input of a staged call: an external wrench (K = ExtWrenchIn), contact normals (NormalsIn) or none (NoSideIn, the plain calls).  What differs
// between the kinds is in their descriptors; which of them a call carries is a template argument, so the plain calls compile to what they were ----

// the staging array of side input K, made when a call first needs it (filled with K's neutral value: a block nobody wrote is no wrench / flat ground)
template <class K>
int ensure_stage_side(srbdqp_handle* h) {
    srbdqp_handle::StagedSide& s = K::staged(h);
    if (s.host) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t count = (size_t)h->stage_h.capacity * K::per_qp(h);
    void* host = nullptr; void* dev = nullptr;
    HIP_TRY(h, hipHostMalloc(&host, count * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    if (hipHostGetDevicePointer(&dev, host, 0) != hipSuccess) {
        (void)hipGetLastError(); (void)hipHostFree(host);
        h->err = std::string("hipHostGetDevicePointer(") + K::staged_label + ") failed";
        return SRBDQP_E_HIP;
    }
    double* v = static_cast<double*>(host);
    for (size_t i = 0; i < count; ++i) v[i] = K::neutral(i);
    s.host = v; s.dev = static_cast<double*>(dev);
    return SRBDQP_OK;
}

// May this handle run staged call `fn` with side input K?  The refusal table answers for the handle's state -- a call that carries a side input admits no form
// but Plain: a side input of the handle in the setters' texts, a live horizon, rank-aware steps --, and K's own rules for what no state bit says: N = 24 has no
// instantiation of K's mode, and only the general kernel reads K (the words of K's setter and of variant_check_batch).
constexpr unsigned kFormsStagedSide = 0;
template <class K>
int check_staged_side(srbdqp_handle* h, const char* fn) {
    if constexpr (K::side == Side::None) return require_form(h, fn, kFormsStaged);
    else {
        if (const int rc = require_form(h, fn, kFormsStagedSide)) return rc;
        if (h->cfg.horizon > row(K::form).max_horizon) { h->err = K::staged_n24(fn); return SRBDQP_E_INVALID; }
        if (!general_allowed(h->cfg)) {
            h->err = std::string(fn) + ": " + row(K::form).noun + " " + K::verb + " read by the general kernel only: srbdqp_config.kernel must be SRBDQP_KERNEL_AUTO or SRBDQP_KERNEL_WRENCH";
            return SRBDQP_E_INVALID;
        }
        return SRBDQP_OK;
    }
}

// B blocks at v (K's staged array, or the caller's own before it is copied there) by the rules of K's setter, before anything is launched
template <class K>
int validate_staged_side(srbdqp_handle* h, const double* v, int32_t B, const char* fn) { return validate<K>(h, v, B, fn, "nothing was launched"); }

// K's staged array as the side input of a call (none: the default)
template <class K>
CallSide call_side(srbdqp_handle* h) {
    if constexpr (K::side == Side::None) return {};
    else return {K::side, K::staged(h).dev, K::staged(h).host};
}

// srbdqp_stage_ext_wrench, srbdqp_stage_contact_normals
template <class K>
int stage_side(srbdqp_handle* h, double** out) {
    if (!h || !out) return SRBDQP_E_INVALID;
    *out = nullptr;
    if (const int rc = ensure_stage_side<K>(h)) return rc;
    *out = K::staged(h).host;
    return SRBDQP_OK;
}

// srbdqp_solve_staged_f64, srbdqp_solve_staged_wrench_f64, srbdqp_solve_staged_normals_f64
template <class K>
int solve_staged(srbdqp_handle* h, const char* fn, int32_t B, int32_t use_pcom, int32_t use_warm, int32_t want_x, int32_t want_y) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = check_staged_side<K>(h, fn)) return rc;
    if (B < 0 || B > h->stage_h.capacity) { h->err = "staged batch exceeds the staging capacity"; return SRBDQP_E_INVALID; }
    if (B == 0) return SRBDQP_OK;
    if constexpr (K::side != Side::None) {
        if (const int rc = ensure_stage_side<K>(h)) return rc;
        if (const int rc = validate_staged_side<K>(h, K::staged(h).host, B, fn)) return rc;
    }
    return solve_staged_impl(h, B, use_pcom, use_warm, want_x, want_y, call_side<K>(h));
}

// srbdqp_update_f64, srbdqp_update_wrench_f64, srbdqp_update_normals_f64 (side: K's array for the one QP; the plain call has none)
template <class K>
int update_staged(srbdqp_handle* h, const char* fn, const double* x0, const double* x_ref, const double* foot, const uint8_t* contact, const double* pcom,
                  const double* side, double* u0_out, double* u_out, double* x_out, int32_t* status, int32_t* iters) {
    constexpr bool with = K::side != Side::None;
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = check_staged_side<K>(h, fn)) return rc;
    if (!x0 || !x_ref || !foot || !contact || (with && !side) || !u0_out) { h->err = "null input/output pointer"; return SRBDQP_E_INVALID; }
    if constexpr (with) if (const int rc = ensure_stage_side<K>(h)) return rc;
    const size_t N = (size_t)h->cfg.horizon;
    const srbdqp_stage& s = h->stage_h;
    if constexpr (with) {
        // the side input first, where the caller has it: a value that is none returns before any staging array -- K's own included -- is written
        if (const int rc = validate_staged_side<K>(h, side, 1, fn)) return rc;
        if (side != K::staged(h).host) std::memcpy(K::staged(h).host, side, K::per_qp(h) * sizeof(double));
    }
    // into the pinned, GPU-mapped staging arrays (2.4 KB at N = 10; an argument that IS the staging array is left where it is)
    if (x0 != s.x0) std::memcpy(s.x0, x0, 13 * sizeof(double));
    if (x_ref != s.x_ref) std::memcpy(s.x_ref, x_ref, N * 13 * sizeof(double));
    if (foot != s.foot) std::memcpy(s.foot, foot, N * 12 * sizeof(double));
    if (contact != s.contact) std::memcpy(s.contact, contact, N * 4);
    if (pcom && pcom != s.pcom) std::memcpy(s.pcom, pcom, N * 3 * sizeof(double));
    // (the plain call through its staged solve's own door, checks included, as it always went; a call with a side input has made its checks above)
    int rc;
    if constexpr (with) rc = solve_staged_impl(h, 1, pcom != nullptr, 0, x_out != nullptr, 0, call_side<K>(h));
    else rc = srbdqp_solve_staged_f64(h, 1, pcom != nullptr, 0, x_out != nullptr, 0);
    if (rc != SRBDQP_OK) return rc;
    if (u0_out != s.u) std::memcpy(u0_out, s.u, 12 * sizeof(double));
    if (u_out && u_out != s.u) std::memcpy(u_out, s.u, N * 12 * sizeof(double));
    if (x_out && x_out != s.x) std::memcpy(x_out, s.x, (N + 1) * 13 * sizeof(double));
    if (status) *status = s.status[0];
    if (iters) *iters = s.iters[0];
    return SRBDQP_OK;
}
}  // namespace

extern "C" {

// the staged calls with their side input: one line each
int srbdqp_solve_staged_f64(srbdqp_handle* h, int32_t B, int32_t use_pcom, int32_t use_warm, int32_t want_x, int32_t want_y) { return solve_staged<NoSideIn>(h, "srbdqp_solve_staged_f64", B, use_pcom, use_warm, want_x, want_y); }
int srbdqp_solve_staged_wrench_f64(srbdqp_handle* h, int32_t B, int32_t use_pcom, int32_t use_warm, int32_t want_x, int32_t want_y) { return solve_staged<ExtWrenchIn>(h, "srbdqp_solve_staged_wrench_f64", B, use_pcom, use_warm, want_x, want_y); }
int srbdqp_solve_staged_normals_f64(srbdqp_handle* h, int32_t B, int32_t use_pcom, int32_t use_warm, int32_t want_x, int32_t want_y) { return solve_staged<NormalsIn>(h, "srbdqp_solve_staged_normals_f64", B, use_pcom, use_warm, want_x, want_y); }
int srbdqp_stage_ext_wrench(srbdqp_handle* h, double** out) { return stage_side<ExtWrenchIn>(h, out); }
int srbdqp_stage_contact_normals(srbdqp_handle* h, double** out) { return stage_side<NormalsIn>(h, out); }
int srbdqp_update_f64(srbdqp_handle* h, const double* x0, const double* x_ref, const double* foot, const uint8_t* contact, const double* pcom, double* u0_out, double* u_out,
                      double* x_out, int32_t* status, int32_t* iters) {
    return update_staged<NoSideIn>(h, "srbdqp_update_f64", x0, x_ref, foot, contact, pcom, nullptr, u0_out, u_out, x_out, status, iters);
}
int srbdqp_update_wrench_f64(srbdqp_handle* h, const double* x0, const double* x_ref, const double* foot, const uint8_t* contact, const double* pcom, const double* ext_wrench,
                             double* u0_out, double* u_out, double* x_out, int32_t* status, int32_t* iters) {
    return update_staged<ExtWrenchIn>(h, "srbdqp_update_wrench_f64", x0, x_ref, foot, contact, pcom, ext_wrench, u0_out, u_out, x_out, status, iters);
}
int srbdqp_update_normals_f64(srbdqp_handle* h, const double* x0, const double* x_ref, const double* foot, const uint8_t* contact, const double* pcom, const double* normals,
                              double* u0_out, double* u_out, double* x_out, int32_t* status, int32_t* iters) {
    return update_staged<NormalsIn>(h, "srbdqp_update_normals_f64", x0, x_ref, foot, contact, pcom, normals, u0_out, u_out, x_out, status, iters);
}

namespace {
KArgs staged_args(srbdqp_handle* h, int32_t B, bool use_pcom, bool want_x, bool want_y) {
    const srbdqp_stage& d = h->stage_d;
    KArgs a = base_args(h->cfg, B, d.x0, d.x_ref, d.foot, d.contact, use_pcom ? d.pcom : nullptr);
    a.u_out = d.u; a.x_out = want_x ? d.x : nullptr; a.y_out = want_y ? d.y : nullptr;
    a.status = d.status; a.iters = d.iters;
    return a;
}
}  // namespace

int srbdqp_prepare_staged_f64(srbdqp_handle* h, int32_t B, int32_t use_pcom) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = require_form(h, "srbdqp_prepare_staged_f64", kFormsTwoPhase)) return rc;
    if (B < 0 || B > h->stage_h.capacity) { h->err = "staged batch exceeds the staging capacity"; return SRBDQP_E_INVALID; }
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    {
        const int rq = aql_quiesce(h);
        if (rq != SRBDQP_OK) return rq;
    }
    const int maxs = plan_two_phase(host_maxs(h, h->stage_h.contact, (size_t)B));
    KArgs a = staged_args(h, B, use_pcom != 0, true, false);
    const int rc = launch_two_phase_any(h, a, h->stream, maxs, 0);
    if (rc != SRBDQP_OK) return rc;
    h->prepared_B = B; h->prepared_maxs = maxs; h->prepared_pcom = use_pcom != 0;
    return SRBDQP_OK;   // asynchronous: the set-up runs behind the handle's stream; srbdqp_solve_prepared_f64 queues behind it
}

int srbdqp_solve_prepared_f64(srbdqp_handle* h, int32_t B, int32_t want_x, int32_t want_y) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = require_form(h, "srbdqp_solve_prepared_f64", kFormsTwoPhase)) return rc;
    if (B <= 0 || B != h->prepared_B) { h->err = "srbdqp_solve_prepared_f64: no set-up of this batch size is pending (srbdqp_prepare_staged_f64)"; return SRBDQP_E_INVALID; }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const bool spin = !(h->cfg.flags & SRBDQP_FLAG_NO_SPIN);
    KArgs a = staged_args(h, B, h->prepared_pcom, want_x != 0, want_y != 0);
    if (spin) { next_seq(h); signal_args(h, a); }
    h->prepared_B = 0;
    h->done_cs = false;            // (the two-phase kernels publish the word without a checksum)
    const int rc = launch_two_phase_any(h, a, h->stream, h->prepared_maxs, 1);
    if (rc != SRBDQP_OK) return rc;
    return wait_done(h, spin);
}

int srbdqp_set_schedule_hint(srbdqp_handle* h, const int32_t* device_iters_prev, int32_t length) {
    if (!h) return SRBDQP_E_INVALID;
    if (device_iters_prev && length < 0) { h->err = "negative hint length"; return SRBDQP_E_INVALID; }
    h->sched_hint = device_iters_prev;
    h->sched_hint_len = device_iters_prev ? (size_t)length : 0;
    return SRBDQP_OK;
}

int srbdqp_set_stamp_buffer(srbdqp_handle* h, void* device_ptr) {
    if (!h) return SRBDQP_E_INVALID;
    h->stamps = reinterpret_cast<long long*>(device_ptr);
    return SRBDQP_OK;
}

int srbdqp_shard_range(int64_t total, int32_t world, int32_t rank, int64_t* first, int64_t* count) {
    if (world < 1 || rank < 0 || rank >= world || total < 0 || !first || !count) return SRBDQP_E_INVALID;
    const int64_t base = total / world, rem = total % world;
    *first = rank * base + (rank < rem ? rank : rem);
    *count = base + (rank < rem ? 1 : 0);
    return SRBDQP_OK;
}

int srbdqp_gather_u0_f64(srbdqp_handle* h, const double* u_local, int64_t B_local, double* u0_all, void* rccl_comm, void* stream) {
    if (!h) return SRBDQP_E_INVALID;
    if (!u_local || !u0_all || !rccl_comm || B_local < 0) { h->err = "srbdqp_gather_u0_f64: null pointer or negative count"; return SRBDQP_E_INVALID; }
    // RCCL by name, once per process: the library does not link it (a single-GPU consumer never needs it)
    struct Rccl {
        int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
        int (*user_rank)(void*, int*) = nullptr;
        int (*count)(void*, int*) = nullptr;
        const char* (*error_string)(int) = nullptr;
        bool ok = false;
        Rccl() {
            void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (!lib) return;
            all_gather = reinterpret_cast<decltype(all_gather)>(dlsym(lib, "ncclAllGather"));
            user_rank = reinterpret_cast<decltype(user_rank)>(dlsym(lib, "ncclCommUserRank"));
            count = reinterpret_cast<decltype(count)>(dlsym(lib, "ncclCommCount"));
            error_string = reinterpret_cast<decltype(error_string)>(dlsym(lib, "ncclGetErrorString"));
            ok = all_gather && user_rank && count;
        }
    };
    static const Rccl rccl;
    if (!rccl.ok) { h->err = "srbdqp_gather_u0_f64: librccl.so.1 (ncclAllGather, ncclCommUserRank, ncclCommCount) is not loadable"; return SRBDQP_E_HIP; }
    auto fail = [&](const char* what, int rc) { h->err = std::string("srbdqp_gather_u0_f64: ") + what + ": " + (rccl.error_string ? rccl.error_string(rc) : "RCCL error"); return SRBDQP_E_HIP; };
    int rank = 0, world = 0, rc;
    if ((rc = rccl.user_rank(rccl_comm, &rank)) != 0) return fail("ncclCommUserRank", rc);
    if ((rc = rccl.count(rccl_comm, &world)) != 0) return fail("ncclCommCount", rc);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
    if (B_local == 0) return SRBDQP_OK;
    double* slot = u0_all + (size_t)rank * (size_t)B_local * 12;
    const long long items = (long long)B_local * 12;
    hipLaunchKernelGGL(srbdqp::srbdqp_pack_u0_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, u_local, slot, items, h->cfg.horizon);
    HIP_TRY(h, hipGetLastError());
    if ((rc = rccl.all_gather(slot, u0_all, (size_t)items, /* ncclDouble */ 8, rccl_comm, st)) != 0) return fail("ncclAllGather", rc);
    return SRBDQP_OK;
}

int srbdqp_flush(srbdqp_handle* h, void* stream) {
    if (!h) return SRBDQP_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (auto& sl : h->slots) {
        if (!sl.used) continue;
        if (stream && sl.st != reinterpret_cast<hipStream_t>(stream)) continue;
        if (const int rc = tail_join(h, sl.rtail, sl.st)) return rc;              // restart passes on the slot's tail stream
        sl.rtail.last = nullptr;
        if (!sl.tail_live) continue;
        const int rc = flush_slot(h, &sl, sl.st);
        if (rc != SRBDQP_OK) return rc;
    }
    return SRBDQP_OK;
}

int srbdqp_synchronize(srbdqp_handle* h) {
    if (!h) return SRBDQP_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->cfg.device));       // (the flush below launches a kernel: a thread that drives several devices may have another one current)
    for (auto& sl : h->slots) {                    // deferred tails of the handle's own stream are part of "everything enqueued"
        if (!sl.used || sl.st != h->stream) continue;
        if (const int rc = tail_join(h, sl.rtail, sl.st)) return rc;
        sl.rtail.last = nullptr;
        if (sl.tail_live) { const int rc = flush_slot(h, &sl, sl.st); if (rc != SRBDQP_OK) return rc; }
    }
    const int rq = aql_quiesce(h);
    if (rq != SRBDQP_OK) return rq;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SRBDQP_OK;
}

double srbdqp_last_kernel_ms(srbdqp_handle* h) {
    if (!h || !h->ev_valid) return -1.0;
    if (hipEventSynchronize(h->ev1) != hipSuccess) return -1.0;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) return -1.0;
    return (double)ms;
}

int srbdqp_last_kernel_parts_ms(srbdqp_handle* h, double* setup_ms, double* admm_ms) {
    if (!h || !setup_ms || !admm_ms) return SRBDQP_E_INVALID;
    if (!h->ev_valid || !h->ev_mid_valid) { h->err = "the last solve was not a timed split-pipeline solve"; return SRBDQP_E_INVALID; }
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    float a = -1.0f, b = -1.0f;
    HIP_TRY(h, hipEventElapsedTime(&a, h->ev0, h->ev_mid));
    HIP_TRY(h, hipEventElapsedTime(&b, h->ev_mid, h->ev1));
    *setup_ms = (double)a; *admm_ms = (double)b;
    return SRBDQP_OK;
}

}  // extern "C"

namespace {

// common body of the host-buffer entry points (esz = sizeof the caller's element type)
int solve_host_impl(srbdqp_handle* h, bool f32, int32_t B, const void* x0, const void* x_ref, const void* foot,
                    const uint8_t* contact, const void* pcom, const void* warm_u, const void* warm_y, void* u_out,
                    void* x_out, void* y_out, int32_t* status, int32_t* iters) {
    if (B < 0 || (B > 0 && (!x0 || !x_ref || !foot || !contact || !u_out))) { h->err = "null input/output pointer"; return SRBDQP_E_INVALID; }
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    {
        const int rq = aql_quiesce(h);
        if (rq != SRBDQP_OK) return rq;
    }
    const size_t N = (size_t)h->cfg.horizon, n = 12 * N, m = 20 * N, b = (size_t)B, esz = f32 ? sizeof(float) : sizeof(double);
    Call c;                        // (no dispatch hint: it belongs to the device-buffer API)
    c.f32 = f32;
    c.plan = plan_solve(h, c, B, host_maxs(h, contact, b));      // the instantiation from the batch's own contact flags
    char *dx0, *dxr, *dft, *dpc, *dwu, *dwy, *du, *dx, *dy; uint8_t* dct; int32_t *dst, *dit;
    return host_call(h, [&](HostIo& io) {
        dx0 = io.in(x0, b * 13 * esz); dxr = io.in(x_ref, b * N * 13 * esz); dft = io.in(foot, b * N * 12 * esz);
        dct = io.in<uint8_t>(contact, b * N * 4);
        dpc = io.in(pcom, b * N * 3 * esz); dwu = io.in(warm_u, b * n * esz); dwy = io.in(warm_y, b * m * esz);
        du = io.out(u_out, b * n * esz); dx = io.out(x_out, b * (N + 1) * 13 * esz); dy = io.out(y_out, b * m * esz);
        dst = io.out<int32_t>(status, b * 4, true); dit = io.out<int32_t>(iters, b * 4, true);
    }, [&](hipStream_t st) {
        int rc = solve_device_impl(h, c, B, dx0, dxr, dft, dct, dpc, dwu, dwy, du, dx, dy, dst, dit, st);
        if (rc == SRBDQP_OK && (h->cfg.flags & SRBDQP_FLAG_DEFER_TAIL)) rc = srbdqp_flush(h, st);   // a host-buffer call returns finished results: whatever was deferred runs now
        return rc;
    });
}

// a device-buffer solve: the dispatch hint applies, the stance-contact bound is the config's (4 where it leaves it open)
Call device_call(const srbdqp_handle* h, bool f32, int32_t B) {
    Call c;
    c.f32 = f32; c.use_hint = true;
    c.plan = plan_solve(h, c, B, maxs_or(h->cfg, 4));
    return c;
}

}  // namespace

extern "C" {

int srbdqp_solve_batch_device_f64(srbdqp_handle* h, int32_t B, const double* x0, const double* x_ref,
                                  const double* foot, const uint8_t* contact, const double* pcom,
                                  const double* warm_u, const double* warm_y, double* u_out, double* x_out,
                                  double* y_out, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = variant_check_batch(h, B)) return rc;
    return solve_device_impl(h, device_call(h, false, B), B, x0, x_ref, foot, contact, pcom, warm_u, warm_y, u_out, x_out, y_out, status, iters, stream);
}

int srbdqp_solve_batch_device_f32(srbdqp_handle* h, int32_t B, const float* x0, const float* x_ref,
                                  const float* foot, const uint8_t* contact, const float* pcom,
                                  const float* warm_u, const float* warm_y, float* u_out, float* x_out,
                                  float* y_out, int32_t* status, int32_t* iters, void* stream) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = require_form(h, "srbdqp_solve_batch_device_f32", kFormsF32)) return rc;
    return solve_device_impl(h, device_call(h, true, B), B, x0, x_ref, foot, contact, pcom, warm_u, warm_y, u_out, x_out, y_out, status, iters, stream);
}

int srbdqp_solve_batch_f64(srbdqp_handle* h, int32_t B, const double* x0, const double* x_ref, const double* foot,
                           const uint8_t* contact, const double* pcom, const double* warm_u, const double* warm_y,
                           double* u_out, double* x_out, double* y_out, int32_t* status, int32_t* iters) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = variant_check_batch(h, B)) return rc;
    return solve_host_impl(h, false, B, x0, x_ref, foot, contact, pcom, warm_u, warm_y, u_out, x_out, y_out, status, iters);
}

int srbdqp_solve_batch_f32(srbdqp_handle* h, int32_t B, const float* x0, const float* x_ref, const float* foot,
                           const uint8_t* contact, const float* pcom, const float* warm_u, const float* warm_y,
                           float* u_out, float* x_out, float* y_out, int32_t* status, int32_t* iters) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = require_form(h, "srbdqp_solve_batch_f32", kFormsF32)) return rc;
    return solve_host_impl(h, true, B, x0, x_ref, foot, contact, pcom, warm_u, warm_y, u_out, x_out, y_out, status, iters);
}

int srbdqp_assemble_f64(srbdqp_handle* h, int32_t B, const double* x0, const double* x_ref, const double* foot,
                        const uint8_t* contact, const double* pcom, double* P_out, double* q_out, double* l_out,
                        double* ub_out) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = require_form(h, "srbdqp_assemble_f64", kFormsAssemble)) return rc;
    if (B < 0 || (B > 0 && (!x0 || !x_ref || !foot || !contact || !P_out || !q_out || !l_out || !ub_out))) { h->err = "null pointer"; return SRBDQP_E_INVALID; }
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t N = (size_t)h->cfg.horizon, n = 12 * N, m = 20 * N, b = (size_t)B;
    Call c;                        // as the host-buffer solve: the instantiation follows the batch's own contact flags
    c.plan = plan_solve(h, c, B, host_maxs(h, contact, b), 0, true);
    if (c.plan.family == Family::General) { h->err = "this configuration solves on the general kernel: use srbdqp_assemble_wrench_f64"; return SRBDQP_E_INVALID; }
    double *dx0, *dxr, *dft, *dpc, *dP, *dq, *dl, *du; uint8_t* dct;
    int rc = host_call(h, [&](HostIo& io) {
        dx0 = io.in<double>(x0, b * 13 * 8); dxr = io.in<double>(x_ref, b * N * 13 * 8); dft = io.in<double>(foot, b * N * 12 * 8);
        dct = io.in<uint8_t>(contact, b * N * 4); dpc = io.in<double>(pcom, b * N * 3 * 8);
        dP = io.zeroed<double>(nullptr, b * n * n * 8); dq = io.zeroed<double>(nullptr, b * n * 8);
        dl = io.zeroed<double>(nullptr, b * m * 8); du = io.zeroed<double>(nullptr, b * m * 8);
    }, [&](hipStream_t st) {
        KArgs a = base_args(h->cfg, B, dx0, dxr, dft, dct, dpc);
        a.P_out = dP; a.q_out = dq; a.l_out = dl; a.ub_out = du;
        a.mode = 1;
        const int rl = launch(h, c, a, st);              // the kernel a solve of this batch would run, stopped before its factorisation
        if (rl != SRBDQP_OK) return rl;
        HIP_TRY(h, hipGetLastError());
        return SRBDQP_OK;
    });
    if (rc != SRBDQP_OK) return rc;
    hipStream_t st = h->stream;
    // compact K, q, map -> full-size P, q in the original variable order (on the host: bookkeeping, not the hot path)
    std::vector<double> K(n * n), qc(n), mp(m);
    const double rho = h->cfg.rho, aa = 4.0 * h->cfg.mu * h->cfg.mu + h->cfg.rho_fz_scale;
    for (size_t q = 0; q < b; ++q) {
        HIP_TRY(h, hipMemcpyAsync(K.data(), dP + q * n * n, n * n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(qc.data(), dq + q * n, n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(mp.data(), dl + q * m, m * 8, hipMemcpyDeviceToHost, st));
        double nad = 0.0;
        HIP_TRY(h, hipMemcpyAsync(&nad, du + q * m, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipStreamSynchronize(st));
        double* P = P_out + q * n * n;
        double* qq = q_out + q * n;
        std::fill(P, P + n * n, 0.0);
        std::fill(qq, qq + n, 0.0);
        if (nad < 0.0) { h->err = "a QP of the batch violates max_contacts_per_step"; return SRBDQP_E_INVALID; }
        const int na = (int)nad, ne = 3 * na;
        if (na == 0) { mp[12 * N] = -srbdqp::kInf; mp[12 * N + 1] = 0.0; }   // flight phase: the kernel leaves before it dumps the friction-row bounds
        for (int r = 0; r < ne; ++r) {
            const int vr = 3 * (int)mp[r / 3] + r % 3;
            qq[vr] = qc[r];
            for (int c = 0; c < ne; ++c) {
                const int vc = 3 * (int)mp[c / 3] + c % 3;
                double v = K[(size_t)r * n + c];
                if (r == c) v -= h->cfg.sigma + rho * ((r % 3 < 2) ? 2.0 : aa);
                P[(size_t)vr * n + vc] = v;
            }
        }
        // a8: rows 20 k + 5 i + j of step k, contact i.  Stance contacts: the bounds the kernel dumped (what its ADMM loop uses);
        // swing contacts were eliminated by the presolve (their rows do not exist on the device): force clamped to 0
        for (size_t k = 0; k < N; ++k)
            for (int i = 0; i < 4; ++i) {
                double* lo = l_out + q * m + 20 * k + 5 * i;
                double* hi = ub_out + q * m + 20 * k + 5 * i;
                for (int j = 0; j < 4; ++j) { lo[j] = mp[12 * N]; hi[j] = mp[12 * N + 1]; }
                lo[4] = 0.0; hi[4] = 0.0;
            }
        for (int e = 0; e < na; ++e) {
            const int gc = (int)mp[e];
            l_out[q * m + 5 * gc + 4] = mp[4 * N + e];
            ub_out[q * m + 5 * gc + 4] = mp[8 * N + e];
        }
    }
    return SRBDQP_OK;
}

int srbdqp_assemble_wrench_f64(srbdqp_handle* h, int32_t B, const double* x0, const double* x_ref, const double* foot,
                               const uint8_t* contact, const double* pcom, double* T_out, double* q_out, double* blocks_out,
                               double* goff_out) {
    if (!h) return SRBDQP_E_INVALID;
    if (const int rc = require_form(h, "srbdqp_assemble_wrench_f64", kFormsAssembleWrench)) return rc;
    if (B < 0 || (B > 0 && (!x0 || !x_ref || !foot || !contact || !T_out || !q_out || !blocks_out || !goff_out))) { h->err = "null pointer"; return SRBDQP_E_INVALID; }
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t N = (size_t)h->cfg.horizon, n = 12 * N, ng = 6 * N, b = (size_t)B;
    double *dx0, *dxr, *dft, *dpc, *dT, *dq, *dbl, *dgo; uint8_t* dct;
    const int rc = host_call(h, [&](HostIo& io) {
        dx0 = io.in<double>(x0, b * 13 * 8); dxr = io.in<double>(x_ref, b * N * 13 * 8); dft = io.in<double>(foot, b * N * 12 * 8);
        dct = io.in<uint8_t>(contact, b * N * 4); dpc = io.in<double>(pcom, b * N * 3 * 8);
        dT = io.zeroed<double>(T_out, b * ng * ng * 8); dq = io.zeroed<double>(q_out, b * n * 8);
        dbl = io.zeroed<double>(blocks_out, b * n * 24 * 8); dgo = io.zeroed<double>(goff_out, b * (N + 1) * 8);
    }, [&](hipStream_t st) {
        KArgs a = base_args(h->cfg, B, dx0, dxr, dft, dct, dpc);
        a.P_out = dT; a.q_out = dq; a.l_out = dbl; a.ub_out = dgo;
        a.mode = 1;
        Call c;
        c.plan = plan_solve(h, c, B, 4, 0, true, true);
        return launch_wrench(h, c, a, st);
    });
    if (rc != SRBDQP_OK) return rc;
    // x0 and the entries of x_ref that are neither yaw nor lever arm enter nothing but the gradient: a solve ends such a QP at its first residual check, and the dump
    // marks it like the QPs the kernel rejects -- here, on the host's copy (the dump kernels stay as they are): goff[N] = -1 and nothing else of the QP written
    for (size_t q = 0; q < b; ++q) {
        double* go = goff_out + q * (N + 1);
        if (go[N] < 0.0) continue;
        bool finite = true;
        for (size_t i = 0; i < n && finite; ++i) finite = std::fabs(q_out[q * n + i]) <= srbdqp::kInf;
        if (finite) continue;
        std::fill(T_out + q * ng * ng, T_out + (q + 1) * ng * ng, 0.0);
        std::fill(q_out + q * n, q_out + (q + 1) * n, 0.0);
        std::fill(blocks_out + q * n * 24, blocks_out + (q + 1) * n * 24, 0.0);
        std::fill(go, go + N, 0.0);
        go[N] = -1.0;
    }
    return SRBDQP_OK;
}

// ---- ragged batches (BASELINE.json configs[4]): mixed horizons, one launch per horizon bucket, all in flight together ----
struct srbdqp_ragged {
    std::vector<srbdqp_handle*> hs;          // one engine (own stream) per horizon bucket
    std::vector<int> horizons;
    std::vector<hipEvent_t> ev_out;
    std::vector<char> ev_out_used;            // ev_out[i] has been recorded by an earlier call
    hipEvent_t ev_in = nullptr;
    bool ev_in_pending = false;
    int device = 0;
    int32_t *h_perm = nullptr, *h_off = nullptr;   // pinned mirrors of a call's bucket permutation and row offsets [rb.items]
    // The device arrays the calls of this object share, as a launch stream of a handle has them: restart sets of rb.items QPs and 20 dual doubles per horizon
    // row, each with the call's index arrays as its two lists.  One set; under SRBDQP_FLAG_DEFER_TAIL kRestartSets in rotation (set = call number mod kRestartSets),
    // and the restart passes of a bucket run on the bucket's own tail stream behind its first pass, beside the next calls.
    RestartBufs rb;
    bool defer = false;
    unsigned long long call_k = 0;
    std::vector<Tail> tails;                  // per bucket (defer only): its closing event per set, and the one srbdqp_ragged_flush waits for
    char* ws = nullptr; size_t ws_bytes = 0;  // host-buffer entry point: device copies of the caller's arrays
    hipStream_t stream = nullptr;             // ... and the stream its copies run on
    // per-QP robot records and cost weights in the caller's QP order (srbdqp_ragged_set_robots, srbdqp_ragged_set_weights / _device), forwarded to every bucket
    // engine: a bucket's workgroup reads the record of the caller's index its dispatch order names
    PerQp<srbdqp_robot> robots;
    PerQp<srbdqp_weights> weights;
    PerQp<double> ext;                     // srbdqp_ragged_set_external_wrench / _device: [rows][6] doubles in the caller's row order (len = rows)
    std::string err;
};

namespace {
std::string g_ragged_err;
}  // namespace

int srbdqp_ragged_create(const srbdqp_config* cfg, const int32_t* horizons, int32_t n_horizons, srbdqp_ragged** out) {
    if (!cfg || !horizons || !out || n_horizons < 1 || n_horizons > 16) { g_ragged_err = "bad argument"; return SRBDQP_E_INVALID; }
    *out = nullptr;
    if (cfg->flags & SRBDQP_FLAG_RANK_AWARE) { g_ragged_err = "SRBDQP_FLAG_RANK_AWARE: ragged objects have no rank-aware form (the flag is read by srbdqp_create's handles only)"; return SRBDQP_E_INVALID; }
    srbdqp_ragged* r = new (std::nothrow) srbdqp_ragged();
    if (!r) { g_ragged_err = "out of host memory"; return SRBDQP_E_NOMEM; }
    r->device = cfg->device;
    auto fail = [&](int rc, const std::string& what) { g_ragged_err = what; srbdqp_ragged_destroy(r); return rc; };
    for (int i = 0; i < n_horizons; ++i) {
        for (int j = 0; j < i; ++j) if (horizons[j] == horizons[i]) return fail(SRBDQP_E_INVALID, "duplicate horizon");
        srbdqp_config c = *cfg;
        c.horizon = horizons[i];
        c.kernel = SRBDQP_KERNEL_WRENCH;       // per-QP contact schedules are free: the general kernel at every horizon
        srbdqp_handle* h = nullptr;
        const int rc = srbdqp_create(&c, &h);
        if (rc != SRBDQP_OK) return fail(rc, std::string("bucket engine: ") + srbdqp_last_error(nullptr));
        r->hs.push_back(h);
        r->horizons.push_back(horizons[i]);
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return fail(SRBDQP_E_HIP, "hipEventCreate");
        r->ev_out.push_back(ev);
        r->ev_out_used.push_back(0);
    }
    if (hipEventCreateWithFlags(&r->ev_in, hipEventDisableTiming) != hipSuccess) return fail(SRBDQP_E_HIP, "hipEventCreate");
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) return fail(SRBDQP_E_HIP, "hipStreamCreate");
    r->defer = (cfg->flags & SRBDQP_FLAG_DEFER_TAIL) != 0;
    if (r->defer) {
        r->tails.resize((size_t)n_horizons);
        for (auto& t : r->tails) if (const int rc = tail_create(r, t)) return fail(rc, r->err);
    }
    *out = r;
    return SRBDQP_OK;
}

int srbdqp_ragged_destroy(srbdqp_ragged* r) {
    if (!r) return SRBDQP_OK;
    (void)hipSetDevice(r->device);
    for (auto* h : r->hs) srbdqp_destroy(h);
    for (auto& t : r->tails) tail_destroy(t);
    for (auto ev : r->ev_out) if (ev) (void)hipEventDestroy(ev);
    if (r->ev_in) (void)hipEventDestroy(r->ev_in);
    if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
    if (r->rb.mem) (void)hipFree(r->rb.mem);
    if (r->h_perm) (void)hipHostFree(r->h_perm);
    if (r->h_off) (void)hipHostFree(r->h_off);
    if (r->ws) (void)hipFree(r->ws);
    r->robots.release(); r->weights.release(); r->ext.release();
    delete r;
    return SRBDQP_OK;
}

const char* srbdqp_ragged_last_error(const srbdqp_ragged* r) { return r ? r->err.c_str() : g_ragged_err.c_str(); }

}  // extern "C"

extern "C" int srbdqp_ragged_flush(srbdqp_ragged* r, void* stream);
namespace {
// a ragged solve of B QPs while side input K is set: fp64 only, and a record for every QP
template <class K>
int ragged_side_check(srbdqp_ragged* r, int32_t B, bool f32) {
    if (K::of(r).dev && f32) {
        r->err = std::string("fp32 ragged solve: refused while ") + K::what + " are set (srbdqp_ragged_set_" + K::name + "): only the fp64 solves read them";
        return SRBDQP_E_INVALID;
    }
    return covers<K>(r, B, "ragged solve of ", " QPs with ", false, true);
}

// common body of the ragged device entry points; esz = element size of the caller's buffers (8 or 4)
int ragged_device_impl(srbdqp_ragged* r, int32_t B, const int32_t* N_per_qp, const void* x0, const void* x_ref, const void* foot,
                       const uint8_t* contact, const void* warm_u, const void* warm_y, void* u_out, void* x_out, void* y_out,
                       int32_t* status, int32_t* iters, void* stream, bool f32) {
    if (!r) return SRBDQP_E_INVALID;
    if (B < 0 || (B > 0 && (!N_per_qp || !x0 || !x_ref || !foot || !contact || !u_out))) { r->err = "null input/output pointer"; return SRBDQP_E_INVALID; }
    if (f32) for (auto* bh : r->hs) if (state_of(bh) & bit(Form::Live)) { const int rc = refuse(bh, Form::Live, "an fp32 ragged solve"); r->err = bh->err; return rc; }
    if (const int rc = ragged_side_check<RobotsIn>(r, B, f32)) return rc;
    if (const int rc = ragged_side_check<WeightsIn>(r, B, f32)) return rc;
    if (r->ext.dev) {   // (its length is in rows: f32 here, the rows of this call below)
        if (const int rc = ragged_side_check<ExtWrenchIn>(r, 0, f32)) return rc;
        long long need = 0;
        for (int32_t b = 0; b < B && N_per_qp; ++b) need += N_per_qp[b];
        if ((size_t)need > r->ext.len) {
            r->err = "ragged solve of " + std::to_string(need) + " horizon rows with an external wrench for " + std::to_string(r->ext.len) + " set: every row needs its wrench";
            return SRBDQP_E_INVALID;
        }
    }
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    hipStream_t sin = stream ? reinterpret_cast<hipStream_t>(stream) : r->stream;
    const size_t nb = r->hs.size();
    // the bucket of every QP (counting sort by horizon) and the rows of the call
    std::vector<int> cnt(nb, 0), start(nb + 1, 0), which((size_t)B);
    long long rows = 0;
    for (int32_t b = 0; b < B; ++b) {
        int k = -1;
        for (size_t i = 0; i < nb; ++i) if (r->horizons[i] == N_per_qp[b]) { k = (int)i; break; }
        if (k < 0) { r->err = "N_per_qp holds a horizon this object was not created for"; return SRBDQP_E_INVALID; }
        which[(size_t)b] = k; ++cnt[(size_t)k];
        if (rows > 2000000000LL) { r->err = "more than 2^31 horizon rows in one call"; return SRBDQP_E_INVALID; }
        rows += N_per_qp[b];
    }
    for (size_t i = 0; i < nb; ++i) start[i + 1] = start[i] + cnt[i];
    bool any_restart = false;
    for (size_t i = 0; i < nb; ++i) any_restart = any_restart || (cnt[i] > 0 && restart_iter_of(r->hs[i]) > 0);
    const int nsets = r->defer ? kRestartSets : 1;
    const size_t duals = any_restart ? 20 * (size_t)rows : 0;                  // (the duals of a pass, for the one behind it: by rows, where everything else is by QPs)
    if (!r->rb.fits((size_t)B, duals, nsets)) {
        // more QPs or more rows than the sets hold: the only point that waits, and only for earlier solves of this object
        for (auto* h : r->hs) HIP_TRY(r, hipStreamSynchronize(h->stream));
        for (auto& t : r->tails) if (const int rc = tail_drain(r, t)) return rc;
        size_t items = r->rb.items;
        if ((size_t)B > items) {                                                 // ... the pinned mirrors with them
            HIP_TRY(r, hipStreamSynchronize(sin));
            if (r->h_perm) (void)hipHostFree(r->h_perm);
            if (r->h_off) (void)hipHostFree(r->h_off);
            r->h_perm = r->h_off = nullptr; r->rb.items = 0;
            items = (size_t)B + (size_t)B / 4 + 64;
            HIP_TRY(r, hipHostMalloc(reinterpret_cast<void**>(&r->h_perm), items * 4, hipHostMallocDefault));
            HIP_TRY(r, hipHostMalloc(reinterpret_cast<void**>(&r->h_off), items * 4, hipHostMallocDefault));
            r->ev_in_pending = false;
        }
        const size_t want_duals = duals > r->rb.duals ? duals + duals / 4 + 64 * 20 : r->rb.duals;
        if (const int rc = carve_restart_sets(r, r->rb, items, want_duals, nsets, 2, 0)) return rc;
    }
    if (r->ev_in_pending) HIP_TRY(r, hipEventSynchronize(r->ev_in));   // the previous call's index upload has left the pinned mirrors
    // the packed row offsets and the bucket permutation
    int32_t row = 0;
    for (int32_t b = 0; b < B; ++b) { r->h_off[b] = row; row += N_per_qp[b]; }
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int32_t b = 0; b < B; ++b) r->h_perm[fill[(size_t)which[(size_t)b]]++] = b;
    // the index arrays (and the restart buffers) are shared by the calls of this object: the upload below must not overtake the
    // bucket kernels of an earlier call made on ANOTHER caller stream (calls on one stream are ordered through ev_out already)
    for (size_t i = 0; i < nb; ++i) if (r->ev_out_used[i]) HIP_TRY(r, hipStreamWaitEvent(sin, r->ev_out[i], 0));
    // this call's set of the shared arrays (deferred restart passes: three in rotation; behind the passes of the set's last user in every bucket)
    const int k = next_set(r->call_k, nsets);
    const RestartSet& set = r->rb.set[k];
    for (auto& t : r->tails) if (const int rc = tail_wait(r, t, k, sin)) return rc;
    int32_t *const d_perm = set.list[0], *const d_off = set.list[1];
    HIP_TRY(r, hipMemcpyAsync(d_off, r->h_off, (size_t)B * 4, hipMemcpyHostToDevice, sin));
    HIP_TRY(r, hipMemcpyAsync(d_perm, r->h_perm, (size_t)B * 4, hipMemcpyHostToDevice, sin));
    HIP_TRY(r, hipEventRecord(r->ev_in, sin));
    r->ev_in_pending = true;
    // one launch per non-empty bucket, each on its engine's own stream behind the upload; the caller's stream then waits for all
    for (size_t i = 0; i < nb; ++i) {
        if (cnt[i] == 0) continue;
        srbdqp_handle* bh = r->hs[i];
        hipStream_t bs = bh->stream;
        Call c;                    // the bucket's plan: the general kernel (srbdqp_ragged_create), in the form the bucket's handle is in
        c.f32 = f32; c.plan = plan_solve(bh, c, cnt[i], 4);
        HIP_TRY(r, hipStreamWaitEvent(bs, r->ev_in, 0));
        KArgs a = base_args(bh->cfg, cnt[i], x0, x_ref, foot, contact);
        a.warm_u = static_cast<const double*>(warm_u); a.warm_y = static_cast<const double*>(warm_y);
        a.u_out = static_cast<double*>(u_out); a.x_out = static_cast<double*>(x_out); a.y_out = static_cast<double*>(y_out);
        a.status = status; a.iters = iters;
        a.perm = d_perm + start[i]; a.row_off = d_off;
        int rcount = 1;
        const int restart = c.plan.restart == Restart::Off ? 0 : restart_iter_of(bh, &rcount);
        // several passes over the bucket, as srbdqp_solve_batch_* does (the later ones select their QPs in-kernel), or one.  Under the defer flag the caller's
        // stream waits for the first pass only: the others run on the bucket's tail stream behind it, beside what the caller enqueues next
        const KArgs a1 = restart > 0 ? first_pass_args(a, restart, set) : a;
        const bool deferred = c.plan.restart == Restart::Deferred;
        auto passes = [&](hipStream_t ps) {
            return run_restart_passes(a1, rcount, bh->cfg.max_iter, set, ps, [&](Pass& pass, int, hipStream_t st) { return launch_wrench(bh, c, pass.a, st); });
        };
        int rc = launch_wrench(bh, c, a1, bs);
        if (rc == SRBDQP_OK && restart > 0 && !deferred) rc = passes(bs);
        if (rc == SRBDQP_OK) {
            HIP_TRY(r, hipEventRecord(r->ev_out[i], bs));
            r->ev_out_used[i] = 1;
            HIP_TRY(r, hipStreamWaitEvent(sin, r->ev_out[i], 0));
            if (deferred) {
                HIP_TRY(r, hipStreamWaitEvent(r->tails[i].st, r->ev_out[i], 0));
                rc = passes(r->tails[i].st);
            }
        }
        if (rc != SRBDQP_OK) { r->err = std::string("bucket N=") + std::to_string(r->horizons[i]) + ": " + bh->err; return rc; }
        if (deferred) if (const int rt = tail_close(r, r->tails[i], k)) return rt;
    }
    return SRBDQP_OK;
}

// common body of the ragged host entry points
int ragged_host_impl(srbdqp_ragged* r, int32_t B, size_t esz, const int32_t* N_per_qp, const void* x0, const void* x_ref, const void* foot,
                     const uint8_t* contact, void* u_out, void* x_out, int32_t* status, int32_t* iters) {
    if (!r) return SRBDQP_E_INVALID;
    if (B < 0 || (B > 0 && (!N_per_qp || !x0 || !x_ref || !foot || !contact || !u_out))) { r->err = "null input/output pointer"; return SRBDQP_E_INVALID; }
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    size_t rows = 0;
    for (int32_t b = 0; b < B; ++b) { if (N_per_qp[b] < 1 || N_per_qp[b] > SRBDQP_MAX_HORIZON) { r->err = "bad horizon in N_per_qp"; return SRBDQP_E_INVALID; } rows += (size_t)N_per_qp[b]; }
    const size_t b = (size_t)B;
    char *dx0, *dxr, *dft, *du, *dx; uint8_t* dct; int32_t *dst, *dit;
    return host_call(r, [&](HostIo& io) {
        dx0 = io.in(x0, b * 13 * esz); dxr = io.in(x_ref, rows * 13 * esz); dft = io.in(foot, rows * 12 * esz); dct = io.in<uint8_t>(contact, rows * 4);
        du = io.out(u_out, rows * 12 * esz); dx = io.out(x_out, (rows + b) * 13 * esz);
        dst = io.out<int32_t>(status, b * 4, true); dit = io.out<int32_t>(iters, b * 4, true);
    }, [&](hipStream_t st) {
        const int rc = ragged_device_impl(r, B, N_per_qp, dx0, dxr, dft, dct, nullptr, nullptr, du, dx, nullptr, dst, dit, st, esz == 4);
        return rc != SRBDQP_OK ? rc : srbdqp_ragged_flush(r, st);   // (deferred restart passes: the copies behind it need every QP finished)
    });
}
}  // namespace

// ---- the setters of the per-QP side inputs (the descriptors RobotsIn, WeightsIn, NormalsIn, ExtWrenchIn above) ----
// One skeleton for the host form and one for the device form, over the kind K and the owner O, a handle or a ragged object.  The owner supplies its device, how
// to quiesce, how to check (owner_check) and what follows a change of the pointer (owner_changed).
namespace {
int owner_device(const srbdqp_handle* h) { return h->cfg.device; }
int owner_device(const srbdqp_ragged* r) { return r->device; }

int quiesce(srbdqp_handle* h) { return quiesce_all_streams(h); }
// every pass that may still read the array this call replaces has completed: the buckets' streams (and their handles' slots), the deferred passes on the tail
// streams, the object's own stream
int quiesce(srbdqp_ragged* r) {
    for (auto* h : r->hs) { const int rq = quiesce_all_streams(h); if (rq != SRBDQP_OK) { r->err = h->err; return rq; } }
    for (auto& t : r->tails) HIP_TRY(r, hipStreamSynchronize(t.st));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return SRBDQP_OK;
}

template <class K> int owner_check(srbdqp_handle* h, const char* fn) { return check_handle<K>(h, fn); }
// may every bucket take it?  (r->err: the bucket's refusal, with the bucket in front unless the text names its live horizon itself)
template <class K> int owner_check(srbdqp_ragged* r, const char*) {
    const std::string fn = std::string(K::what) + " on a ragged object";
    for (auto* bh : r->hs)
        if (const int rc = check_handle<K>(bh, fn.c_str())) {
            r->err = (bh->live_nstar ? std::string() : "bucket N=" + std::to_string(bh->cfg.horizon) + ": ") + bh->err;
            return rc;
        }
    return SRBDQP_OK;
}

template <class K, class O> int set_device(O* o, const char* fn, const typename K::T* dev, int32_t length);
template <class K> int owner_changed(srbdqp_handle*) { return SRBDQP_OK; }
// the buckets read the object's array: the device setter of every bucket engine
template <class K> int owner_changed(srbdqp_ragged* r) {
    const std::string fn = std::string("srbdqp_set_") + K::name + "_device";
    for (size_t i = 0; i < r->hs.size(); ++i) {
        const int rc = set_device<K>(r->hs[i], fn.c_str(), K::of(r).dev, (int32_t)K::of(r).len);
        if (rc != SRBDQP_OK) { r->err = std::string("bucket N=") + std::to_string(r->horizons[i]) + ": " + r->hs[i]->err; return rc; }
    }
    return SRBDQP_OK;
}

// The host form: the library's own device copy.  Clearing (NULL with any length, or length 0) is accepted in every state; an invalid array leaves the previous
// setting as it was; a failed allocation leaves the owner cleared.
template <class K, class O>
int set_host(O* o, const char* fn, const typename K::T* host, int32_t length) {
    if (!o) return SRBDQP_E_INVALID;
    if (host && length < 0) { o->err = std::string(fn) + ": negative length"; return SRBDQP_E_INVALID; }
    const bool clear = !host || length == 0;
    if (!clear) {
        int rv = owner_check<K>(o, fn);
        if (rv == SRBDQP_OK) rv = validate<K>(o, host, length, fn);
        if (rv != SRBDQP_OK) return rv;
    }
    HIP_TRY(o, hipSetDevice(owner_device(o)));
    int rc = quiesce(o);                            // (deferred passes may still read the array this call replaces)
    if (rc != SRBDQP_OK) return rc;
    PerQp<typename K::T>& s = K::of(o);
    if (clear) { s.clear(); return owner_changed<K>(o); }
    const size_t want = (size_t)length * K::per_qp(o);
    if (want > s.cap) { s.clear(); (void)owner_changed<K>(o); }   // (grow frees the old copy: nobody reads it from here on)
    rc = grow(o, s.own, s.cap, want, nullptr, K::alloc);
    if (rc != SRBDQP_OK) return rc;
    HIP_TRY(o, hipMemcpy(s.own, host, sizeof(typename K::T) * want, hipMemcpyHostToDevice));
    s.dev = s.own; s.len = (size_t)length;
    return owner_changed<K>(o);
}

// The device form: the caller's array, which the caller keeps alive and unchanged while solves read it -- no device call, no wait.
template <class K, class O>
int set_device(O* o, const char* fn, const typename K::T* dev, int32_t length) {
    if (!o) return SRBDQP_E_INVALID;
    if (dev && length < 0) { o->err = std::string(fn) + ": negative length"; return SRBDQP_E_INVALID; }
    const bool clear = !dev || length == 0;
    if (!clear) if (const int rc = owner_check<K>(o, fn)) return rc;
    PerQp<typename K::T>& s = K::of(o);
    s.dev = clear ? nullptr : dev;
    s.len = clear ? 0 : (size_t)length;
    return owner_changed<K>(o);
}
}  // namespace

extern "C" {

int srbdqp_set_robots(srbdqp_handle* h, const srbdqp_robot* host, int32_t length) { return set_host<RobotsIn>(h, "srbdqp_set_robots", host, length); }
int srbdqp_set_robots_device(srbdqp_handle* h, const srbdqp_robot* dev, int32_t length) { return set_device<RobotsIn>(h, "srbdqp_set_robots_device", dev, length); }
int srbdqp_set_weights(srbdqp_handle* h, const srbdqp_weights* host, int32_t length) { return set_host<WeightsIn>(h, "srbdqp_set_weights", host, length); }
int srbdqp_set_weights_device(srbdqp_handle* h, const srbdqp_weights* dev, int32_t length) { return set_device<WeightsIn>(h, "srbdqp_set_weights_device", dev, length); }
int srbdqp_set_contact_normals(srbdqp_handle* h, const double* host, int32_t length) { return set_host<NormalsIn>(h, "srbdqp_set_contact_normals", host, length); }
int srbdqp_set_contact_normals_device(srbdqp_handle* h, const double* dev, int32_t length) { return set_device<NormalsIn>(h, "srbdqp_set_contact_normals_device", dev, length); }
int srbdqp_ragged_set_robots(srbdqp_ragged* r, const srbdqp_robot* host, int32_t length) { return set_host<RobotsIn>(r, "srbdqp_ragged_set_robots", host, length); }
int srbdqp_ragged_set_robots_device(srbdqp_ragged* r, const srbdqp_robot* dev, int32_t length) { return set_device<RobotsIn>(r, "srbdqp_ragged_set_robots_device", dev, length); }
int srbdqp_ragged_set_weights(srbdqp_ragged* r, const srbdqp_weights* host, int32_t length) { return set_host<WeightsIn>(r, "srbdqp_ragged_set_weights", host, length); }
int srbdqp_ragged_set_weights_device(srbdqp_ragged* r, const srbdqp_weights* dev, int32_t length) { return set_device<WeightsIn>(r, "srbdqp_ragged_set_weights_device", dev, length); }
int srbdqp_set_external_wrench(srbdqp_handle* h, const double* host, int32_t length) { return set_host<ExtWrenchIn>(h, "srbdqp_set_external_wrench", host, length); }
int srbdqp_set_external_wrench_device(srbdqp_handle* h, const double* dev, int32_t length) { return set_device<ExtWrenchIn>(h, "srbdqp_set_external_wrench_device", dev, length); }
int srbdqp_ragged_set_external_wrench(srbdqp_ragged* r, const double* host, int32_t rows) { return set_host<ExtWrenchIn>(r, "srbdqp_ragged_set_external_wrench", host, rows); }
int srbdqp_ragged_set_external_wrench_device(srbdqp_ragged* r, const double* dev, int32_t rows) { return set_device<ExtWrenchIn>(r, "srbdqp_ragged_set_external_wrench_device", dev, rows); }

int srbdqp_ragged_flush(srbdqp_ragged* r, void* stream) {
    if (!r) return SRBDQP_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    hipStream_t sin = stream ? reinterpret_cast<hipStream_t>(stream) : r->stream;
    // (the events stay: they are re-recorded by every call, waiting for a completed one costs nothing, and a caller that issued calls on two streams
    //  flushes each of them -- a flush of the other stream must still find the passes that write ITS outputs)
    for (auto& t : r->tails) if (const int rc = tail_join(r, t, sin)) return rc;
    return SRBDQP_OK;
}

int srbdqp_solve_ragged_device_f64(srbdqp_ragged* r, int32_t B, const int32_t* N_per_qp, const double* x0, const double* x_ref,
                                   const double* foot, const uint8_t* contact, double* u_out, double* x_out, int32_t* status,
                                   int32_t* iters, void* stream) {
    return ragged_device_impl(r, B, N_per_qp, x0, x_ref, foot, contact, nullptr, nullptr, u_out, x_out, nullptr, status, iters, stream, false);
}

int srbdqp_solve_ragged_device_f32(srbdqp_ragged* r, int32_t B, const int32_t* N_per_qp, const float* x0, const float* x_ref,
                                   const float* foot, const uint8_t* contact, float* u_out, float* x_out, int32_t* status,
                                   int32_t* iters, void* stream) {
    return ragged_device_impl(r, B, N_per_qp, x0, x_ref, foot, contact, nullptr, nullptr, u_out, x_out, nullptr, status, iters, stream, true);
}

int srbdqp_solve_ragged_warm_device_f64(srbdqp_ragged* r, int32_t B, const int32_t* N_per_qp, const double* x0, const double* x_ref,
                                        const double* foot, const uint8_t* contact, const double* warm_u, const double* warm_y,
                                        double* u_out, double* x_out, double* y_out, int32_t* status, int32_t* iters, void* stream) {
    return ragged_device_impl(r, B, N_per_qp, x0, x_ref, foot, contact, warm_u, warm_y, u_out, x_out, y_out, status, iters, stream, false);
}

int srbdqp_solve_ragged_warm_device_f32(srbdqp_ragged* r, int32_t B, const int32_t* N_per_qp, const float* x0, const float* x_ref,
                                        const float* foot, const uint8_t* contact, const float* warm_u, const float* warm_y,
                                        float* u_out, float* x_out, float* y_out, int32_t* status, int32_t* iters, void* stream) {
    return ragged_device_impl(r, B, N_per_qp, x0, x_ref, foot, contact, warm_u, warm_y, u_out, x_out, y_out, status, iters, stream, true);
}

int srbdqp_solve_ragged_f64(srbdqp_ragged* r, int32_t B, const int32_t* N_per_qp, const double* x0, const double* x_ref,
                            const double* foot, const uint8_t* contact, double* u_out, double* x_out, int32_t* status, int32_t* iters) {
    return ragged_host_impl(r, B, sizeof(double), N_per_qp, x0, x_ref, foot, contact, u_out, x_out, status, iters);
}

int srbdqp_solve_ragged_f32(srbdqp_ragged* r, int32_t B, const int32_t* N_per_qp, const float* x0, const float* x_ref,
                            const float* foot, const uint8_t* contact, float* u_out, float* x_out, int32_t* status, int32_t* iters) {
    return ragged_host_impl(r, B, sizeof(float), N_per_qp, x0, x_ref, foot, contact, u_out, x_out, status, iters);
}

}  // extern "C"

// ---- the steps either side of the QP (include/srbdqp_cascade.h) --------------------------------------------------
namespace {
inline unsigned elementwise_grid(long long B) {
    // grid-stride kernels: enough 256-thread workgroups to fill 256 CUs several times over, no more
    const long long want = (B + 255) / 256;
    return (unsigned)(want < 1 ? 1 : (want > 256 * 16 ? 256 * 16 : want));
}

// how every check of this section starts: no handle, then the null test of a call over B items (B = 0: nothing to do, no array needed; `missing`: an array
// the call needs is NULL)
int arrays_check(srbdqp_handle* h, bool B_in_range, int64_t B, bool missing) {
    if (!h) return SRBDQP_E_INVALID;
    if (!B_in_range || (B > 0 && missing)) { h->err = "null input/output pointer"; return SRBDQP_E_INVALID; }
    return SRBDQP_OK;
}

int swing_check(srbdqp_handle* h, int64_t B, const void* p_start, const void* p_final, const void* z_middle, const void* progress, const void* pos) {
    return arrays_check(h, B >= 0, B, !p_start || !p_final || !z_middle || !progress || !pos);
}

int wbid_reference_check(srbdqp_handle* h, int64_t B, const void* x_next, const void* u0, const void* foot, const void* R, const void* base_vel,
                         const void* base_acc, const void* com_acc) {
    return arrays_check(h, B >= 0, B, !x_next || !u0 || !foot || !R || !base_vel || !base_acc || !com_acc);
}

// the gait rule: what is wrong with a gait (null: nothing), in the words its callers put behind their own
#define SRBDQP_GAIT_RULE "(struct_size, 1 <= period_steps, 0 <= double_support_steps <= period_steps)"
const char* gait_fault(const srbdqp_gait* g) {
    return !g || g->struct_size != (int32_t)sizeof(srbdqp_gait) || g->period_steps < 1 || g->double_support_steps < 0 || g->double_support_steps > g->period_steps
               ? SRBDQP_GAIT_RULE : nullptr;
}
}  // namespace

extern "C" {

int srbdqp_swing_device_f64(srbdqp_handle* h, int64_t B, const double* p_start, const double* p_final,
                            const double* z_middle, const double* progress, double final_velocity_z,
                            double first_half_share, double* pos, double* vel_z, double* acc_z, double* coeff,
                            void* stream) {
    if (const int rc = swing_check(h, B, p_start, p_final, z_middle, progress, pos)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    srbdqp::SwingArgs a{p_start, p_final, z_middle, progress, pos, vel_z, acc_z, coeff, final_velocity_z, first_half_share, (long long)B};
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
    hipLaunchKernelGGL(srbdqp::srbdqp_swing_kernel, dim3(elementwise_grid(B)), dim3(256), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    h->kname = "swing_f64";
    return SRBDQP_OK;
}

int srbdqp_swing_f64(srbdqp_handle* h, int64_t B, const double* p_start, const double* p_final, const double* z_middle,
                     const double* progress, double final_velocity_z, double first_half_share, double* pos,
                     double* vel_z, double* acc_z, double* coeff) {
    if (const int rc = swing_check(h, B, p_start, p_final, z_middle, progress, pos)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)B;
    double *ds, *df, *dm, *dt, *dp, *dv, *da, *dc;
    return host_call(h, [&](HostIo& io) {
        ds = io.in<double>(p_start, b * 24); df = io.in<double>(p_final, b * 24); dm = io.in<double>(z_middle, b * 8); dt = io.in<double>(progress, b * 8);
        dp = io.out<double>(pos, b * 24); dv = io.out<double>(vel_z, b * 8); da = io.out<double>(acc_z, b * 8); dc = io.out<double>(coeff, b * 56);
    }, [&](hipStream_t st) { return srbdqp_swing_device_f64(h, B, ds, df, dm, dt, final_velocity_z, first_half_share, dp, dv, da, dc, st); });
}

int srbdqp_wbid_reference_device_f64(srbdqp_handle* h, int64_t B, const double* x_next, const double* u0,
                                     const double* foot, int32_t as_written, double* R, double* base_vel,
                                     double* base_acc, double* com_acc, void* stream) {
    if (const int rc = wbid_reference_check(h, B, x_next, u0, foot, R, base_vel, base_acc, com_acc)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    srbdqp::WbidRefArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x_next = x_next; a.u0 = u0; a.foot = foot; a.R = R; a.base_vel = base_vel; a.base_acc = base_acc; a.com_acc = com_acc;
    for (int i = 0; i < 3; ++i) a.iinv[i] = 1.0 / h->cfg.inertia[i];
    a.mass = h->cfg.mass;
    // robot b's own mass and inertia (srbdqp_set_robots): the fleet chain stays consistent with the QPs it solved
    if (const int rc = covers<RobotsIn>(h, B, "srbdqp_wbid_reference: ", " robots with ", false, false)) return rc;
    a.robots = reinterpret_cast<const double*>(h->robots.dev);
    a.gravity = -9.80665;   // wbid.py:286
    a.as_written = as_written ? 1 : 0;
    a.B = (long long)B;
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
    hipLaunchKernelGGL(srbdqp::srbdqp_wbid_reference_kernel, dim3(elementwise_grid(B)), dim3(256), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    h->kname = "wbid_reference_f64";
    return SRBDQP_OK;
}

int srbdqp_wbid_reference_f64(srbdqp_handle* h, int64_t B, const double* x_next, const double* u0, const double* foot,
                              int32_t as_written, double* R, double* base_vel, double* base_acc, double* com_acc) {
    if (const int rc = wbid_reference_check(h, B, x_next, u0, foot, R, base_vel, base_acc, com_acc)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)B;
    double *dx, *du, *df, *dR, *dv, *da, *dc;
    return host_call(h, [&](HostIo& io) {
        dx = io.in<double>(x_next, b * 13 * 8); du = io.in<double>(u0, b * 12 * 8); df = io.in<double>(foot, b * 12 * 8);
        dR = io.out<double>(R, b * 9 * 8); dv = io.out<double>(base_vel, b * 6 * 8); da = io.out<double>(base_acc, b * 6 * 8); dc = io.out<double>(com_acc, b * 3 * 8);
    }, [&](hipStream_t st) { return srbdqp_wbid_reference_device_f64(h, B, dx, du, df, as_written, dR, dv, da, dc, st); });
}

}  // extern "C"

// ---- from step t to step t + 1: the fleet's plant step and the K-step loop (include/srbdqp_cascade.h; the kernel: srbdqp_fleet.hpp) ----------------------
namespace {

// what is wrong with a settings struct (null: nothing)
const char* fleet_settings_fault(const srbdqp_fleet_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_fleet_settings)) return "struct_size is not sizeof(srbdqp_fleet_settings)";
    if (s->substeps < 1 || s->substeps > 1000) return "1 <= substeps <= 1000";
    for (const double v : {s->foot_half_length, s->z_min, s->tilt_max})
        if (!std::isfinite(v) || !(v > 0.0)) return "foot_half_length, z_min and tilt_max must be finite and positive";
    return gait_fault(&s->gait) ? "invalid gait " SRBDQP_GAIT_RULE : nullptr;
}

// the roll-out's records of one period (srbdqp::FleetArgs): all null outside a roll-out
struct FleetLogs {
    double *x = nullptr, *feet = nullptr, *u0 = nullptr;
    const int32_t *status = nullptr, *iters = nullptr;
    int32_t *status_log = nullptr, *iters_log = nullptr;
};

// one launch of the plant step; the arguments have been checked.  landing_yaw null: feet land unturned
int fleet_advance_launch(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride, const double* landing,
                         const double* landing_yaw, const uint8_t* standing, const double* push, uint8_t* alive, const srbdqp_fleet_settings* cfg,
                         const FleetLogs& lg, hipStream_t st) {
    srbdqp::FleetArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.feet = feet; a.stamp = stamp; a.u0 = u0; a.u0_stride = (long long)u0_stride; a.landing = landing; a.standing = standing; a.push = push;
    a.alive = alive;
    a.robots = reinterpret_cast<const double*>(h->robots.dev);   // robot b's own mass and inertia: the plant of the QP it solved
    a.x_log = lg.x; a.feet_log = lg.feet; a.u0_log = lg.u0; a.status = lg.status; a.iters = lg.iters;
    a.status_log = lg.status ? lg.status_log : nullptr; a.iters_log = lg.iters ? lg.iters_log : nullptr;
    a.mass = h->cfg.mass;
    for (int i = 0; i < 3; ++i) a.inertia[i] = h->cfg.inertia[i];
    a.dt = h->cfg.dt; a.foot_half_length = cfg->foot_half_length; a.z_min = cfg->z_min; a.tilt_max = cfg->tilt_max;
    a.substeps = cfg->substeps; a.period = cfg->gait.period_steps; a.ds = cfg->gait.double_support_steps;
    a.B = (long long)B;
    const srbdqp::TerrainMap* map = h->terrain.map.h ? &h->terrain.map : nullptr;   // a map set: the terrain instantiation over it
    HIP_TRY(h, srbdqp::launch_fleet_advance(a, st, map, landing_yaw));   // landing_yaw: the steered instantiation, feet turned by it
    h->kname = landing_yaw ? (map ? "fleet_advance_terrain_steered_f64" : "fleet_advance_steered_f64") : (map ? "fleet_advance_terrain_f64" : "fleet_advance_f64");
    return SRBDQP_OK;
}

// steered: the call is srbdqp_fleet_advance_steered_*, which needs the landing_yaw that the plain call does not take
int fleet_advance_check(srbdqp_handle* h, int64_t B, const void* x, const void* feet, const void* stamp, const void* u0, int64_t u0_stride, const void* landing,
                        const void* landing_yaw, bool steered, const srbdqp_fleet_settings* cfg) {
    if (const int rc = arrays_check(h, B >= 0, B, !x || !feet || !stamp || !u0 || !landing)) return rc;
    if (u0_stride < 12) { h->err = "srbdqp_fleet_advance: u0_stride must be at least 12 doubles"; return SRBDQP_E_INVALID; }
    if (const char* why = fleet_settings_fault(cfg)) { h->err = std::string("invalid srbdqp_fleet_settings: ") + why; return SRBDQP_E_INVALID; }
    if (const int rc = covers<RobotsIn>(h, B, "srbdqp_fleet_advance: ", " robots with ", false, false)) return rc;
    if (steered && B > 0 && !landing_yaw) { h->err = "srbdqp_fleet_advance_steered: landing_yaw is NULL (srbdqp_mpc_inputs_steered_* writes it; srbdqp_fleet_advance_* lands feet unturned)"; return SRBDQP_E_INVALID; }
    return SRBDQP_OK;
}

// the plant step behind its four entry points: device buffers, then host buffers staged around the same call
int fleet_advance_device(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride, const double* landing,
                         const double* landing_yaw, bool steered, const uint8_t* standing, const double* push, uint8_t* alive, const srbdqp_fleet_settings* cfg,
                         void* stream) {
    if (const int rc = fleet_advance_check(h, B, x, feet, stamp, u0, u0_stride, landing, landing_yaw, steered, cfg)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
    return fleet_advance_launch(h, B, x, feet, stamp, u0, u0_stride, landing, landing_yaw, standing, push, alive, cfg, FleetLogs{}, st);
}

int fleet_advance_host(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride, const double* landing,
                       const double* landing_yaw, bool steered, const uint8_t* standing, const double* push, uint8_t* alive, const srbdqp_fleet_settings* cfg) {
    if (const int rc = fleet_advance_check(h, B, x, feet, stamp, u0, u0_stride, landing, landing_yaw, steered, cfg)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)B;
    double *dx, *dfe, *dst, *du, *dlp, *dly, *dpu;
    uint8_t *dsd, *dal;
    return host_call(h, [&](HostIo& io) {
        dx = io.add<double>(x, x, b * 13 * 8, false); dfe = io.add<double>(feet, feet, b * 12 * 8, false); dst = io.add<double>(stamp, stamp, b * 8, false);
        du = io.in<double>(u0, ((b - 1) * (size_t)u0_stride + 12) * 8); dlp = io.in<double>(landing, b * 3 * 8); dly = io.in<double>(landing_yaw, b * 8);
        dsd = io.in<uint8_t>(standing, b); dpu = io.in<double>(push, b * 6 * 8);
        dal = alive ? io.add<uint8_t>(alive, alive, b, false) : nullptr;
    }, [&](hipStream_t st) { return fleet_advance_device(h, B, dx, dfe, dst, du, u0_stride, dlp, dly, steered, dsd, dpu, dal, cfg, st); });
}

// ---- a fleet that steers (include/srbdqp_cascade.h; the kernel: srbdqp_steer.hpp) ----
// a call refused before its handle is looked at leaves its reason where srbdqp_last_error(NULL) reads it
int steer_refuse(srbdqp_handle* h, const std::string& why) { (h ? h->err : g_create_err) = why; return SRBDQP_E_INVALID; }

// the first entry of a HOST array of commands that is not finite, or -1
long long steer_non_finite(const double* command, size_t count) {
    for (size_t i = 0; i < count; ++i) if (!std::isfinite(command[i])) return (long long)i;
    return -1;
}

// ---- a fleet that follows its path (include/srbdqp_cascade.h; the kernel: srbdqp_steer.hpp) ----
// what is wrong with a tracked call's settings (null: nothing)
const char* track_settings_fault(const srbdqp_track_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_track_settings)) return "struct_size is not sizeof(srbdqp_track_settings)";
    for (const double v : {s->lead_max, s->yaw_lead_max})
        if (!std::isfinite(v) || !(v > 0.0)) return "lead_max and yaw_lead_max must be finite and positive";
    return nullptr;
}

// what a tracked call checks before its handle is looked at: the settings, the pose, and in a host form that pose [B][3] and command [rows][B][3] are finite.
// fn: the call, for the texts
int track_check(srbdqp_handle* h, const char* fn, int64_t B, const srbdqp_track_settings* trk, const double* pose, const double* command, size_t rows, bool host) {
    const std::string who = fn;
    if (const char* why = track_settings_fault(trk)) return steer_refuse(h, who + ": invalid srbdqp_track_settings: " + why);
    if (!pose && B > 0) return steer_refuse(h, who + ": pose is NULL ([B][3] = (qx, qy, th) goes in and out: (x[3], x[4], x[2]) starts on the robot)");
    if (host && B >= 1 && B <= 0x7fffffffLL) {
        long long i = steer_non_finite(pose, (size_t)B * 3);
        if (i >= 0) return steer_refuse(h, who + ": the pose of robot " + std::to_string(i / 3) + " is not finite (component " + std::to_string(i % 3) + " of qx, qy, th)");
        i = command ? steer_non_finite(command, rows * (size_t)B * 3) : -1;
        if (i >= 0) return steer_refuse(h, who + ": the command of robot " + std::to_string((i / 3) % B) + (rows > 1 ? " at row " + std::to_string(i / (3 * B)) : std::string()) + " is not finite");
    }
    return SRBDQP_OK;
}

// ---- footholds previewed along the horizon (include/srbdqp_cascade.h; the kernel: srbdqp_steer.hpp) ----
// what is wrong with a previewed call's settings (null: nothing)
const char* preview_settings_fault(const srbdqp_preview_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_preview_settings)) return "struct_size is not sizeof(srbdqp_preview_settings)";
    if (!std::isfinite(s->foot_half_length) || !(s->foot_half_length > 0.0)) return "foot_half_length must be finite and positive";
    return nullptr;
}

// ---- the step before the QP: one argument record, one check, one launch, one device path, one host path for the eight srbdqp_mpc_inputs* entry points ----
// the flavours of an inputs call (kSteered, kTracked, kPreview) and of a roll-out (all four).  kTracked: beside kSteered, the inputs call is the tracked one
// (section 21); kPreview: beside kSteered, with or without kTracked, foot holds the footholds previewed along the horizon (section 22)
enum : unsigned { kObserved = 1u, kSteered = 2u, kTracked = 4u, kPreview = 8u };

// the arguments of an inputs call, as its entry point got them: device addresses, or the caller's host arrays (mpc_inputs_host).  What a flavour does not
// read stands last and stays null
struct InputsArgs {
    unsigned flavour;                  // 0: srbdqp_mpc_inputs_*; kSteered: ..._steered_*; kSteered | kTracked: ..._tracked_*; with kPreview: ..._previewed_*
    const char* fn;                    // the call, for error texts
    int64_t B;
    const double *x0, *feet, *stamp;
    const double* vel;                 // v_ref [B][2]; steered: command [B][3]
    const uint8_t* standing; const srbdqp_gait* gait;
    double *x_ref, *foot; uint8_t* contact; double *pcom, *landing;
    double* landing_yaw;               // written by a steered call; null otherwise
    const srbdqp_track_settings* trk; double *pose, *pose_log;    // read in a tracked call only; pose_log: the row of a roll-out's log, or null
    const srbdqp_preview_settings* prv; uint8_t* previewed;       // read in a previewed call only; previewed [B][N][4] or null
};

// what MpcInputsArgs and SteerInputsArgs share, under the same names
template <class A>
void inputs_fill(A& a, const srbdqp_handle* h, const InputsArgs& c) {
    std::memset(&a, 0, sizeof(a));
    a.x0 = c.x0; a.feet = c.feet; a.stamp = c.stamp; a.standing = c.standing;
    a.x_ref = c.x_ref; a.foot = c.foot; a.contact = c.contact; a.pcom = c.pcom; a.landing = c.landing;
    for (int i = 0; i < 3; ++i) a.com_target[i] = c.gait->com_target[i];
    a.hip_offset_y = c.gait->hip_offset_y; a.dt = h->cfg.dt;
    a.N = h->cfg.horizon; a.period = c.gait->period_steps; a.ds = c.gait->double_support_steps;
    a.B = (long long)c.B;
}

// one launch of the inputs; the arguments have been checked
int mpc_inputs_launch(srbdqp_handle* h, const InputsArgs& c, hipStream_t st) {
    if (c.flavour & kSteered) {        // from command [B][3]: the commanded kernel of the second code object, tracked with the pose as its second argument
        const bool tracked = c.flavour & kTracked;
        srbdqp::SteerInputsArgs a;
        inputs_fill(a, h, c);
        a.command = c.vel; a.landing_yaw = c.landing_yaw;
        const srbdqp::TrackPose tp = tracked ? srbdqp::TrackPose{c.pose, c.pose_log, c.trk->lead_max, c.trk->yaw_lead_max} : srbdqp::TrackPose{};
        const bool preview = c.flavour & kPreview;
        const srbdqp::PreviewFeet pf = preview ? srbdqp::PreviewFeet{c.previewed, c.prv->foot_half_length} : srbdqp::PreviewFeet{};
        HIP_TRY(h, srbdqp::launch_mpc_inputs_commanded(a, tracked ? &tp : nullptr, h->live_nstar != 0, st, preview ? &pf : nullptr));
        h->kname = preview ? (tracked ? "mpc_inputs_tracked_previewed_f64" : "mpc_inputs_previewed_f64") : (tracked ? "mpc_inputs_tracked_f64" : "mpc_inputs_steered_f64");
        return SRBDQP_OK;
    }
    srbdqp::MpcInputsArgs a;           // from v_ref [B][2]: the kernel of this code object
    inputs_fill(a, h, c);
    a.v_ref = c.vel;
    const long long tiles = ((long long)c.B + 31) / 32;                 // one tile of 32 robots per workgroup pass
    const dim3 grid((unsigned)(tiles < 1 ? 1 : (tiles > 256 * 32 ? 256 * 32 : tiles)));
    int rc = SRBDQP_OK;
    if (h->live_nstar) hipLaunchKernelGGL(srbdqp::srbdqp_mpc_inputs_kernel<0>, grid, dim3(256), 0, st, a);   // (a live horizon: a.N at run time)
    else rc = with_horizon(h, [&](auto n) -> int {
        hipLaunchKernelGGL(srbdqp::srbdqp_mpc_inputs_kernel<decltype(n)::value>, grid, dim3(256), 0, st, a);
        return SRBDQP_OK;
    });
    if (rc != SRBDQP_OK) return rc;
    HIP_TRY(h, hipGetLastError());
    h->kname = "mpc_inputs_f64";
    return SRBDQP_OK;
}

// where an inputs call stands: on device addresses, on the caller's host arrays, or on device addresses behind mpc_inputs_host's staging
enum class InputsFrom { Device, Host, Staged };

// May this handle run this inputs call?  In order:
//  * the command's own rules (tracked: the pose's and the settings' too), which need no handle and come first; on host arrays every entry must be finite.
//    Behind the staging they have been decided on the caller's arrays already;
//  * the arrays, and in a steered call B <= 2^31 - 1;
//  * the gait -- which the v_ref host form leaves to the device form behind its staging, as it always has: B = 0 is OK with any gait there
int mpc_inputs_check(srbdqp_handle* h, const InputsArgs& c, InputsFrom from) {
    const bool steered = c.flavour & kSteered, host = from == InputsFrom::Host;
    if (c.flavour & kPreview) if (const char* why = preview_settings_fault(c.prv)) return steer_refuse(h, std::string(c.fn) + ": invalid srbdqp_preview_settings: " + why);
    if (c.flavour & kTracked) {
        if (from != InputsFrom::Staged) if (const int rc = track_check(h, c.fn, c.B, c.trk, c.pose, c.vel, 1, host)) return rc;
    } else if (steered && host && c.B > 0 && c.B <= 0x7fffffffLL && c.vel) {
        const long long i = steer_non_finite(c.vel, (size_t)c.B * 3);
        if (i >= 0) return steer_refuse(h, std::string(c.fn) + ": the command of robot " + std::to_string(i / 3) + " is not finite (component " + std::to_string(i % 3) + " of vx, vy, wz)");
    }
    if (const int rc = arrays_check(h, c.B >= 0 && !(steered && c.B > 0x7fffffffLL), c.B,
                                    !c.x0 || !c.feet || !c.stamp || !c.vel || !c.x_ref || !c.foot || !c.contact || !c.pcom)) return rc;
    if (const char* why = (steered || !host) ? gait_fault(c.gait) : nullptr) { h->err = std::string("invalid srbdqp_gait ") + why; return SRBDQP_E_INVALID; }
    return SRBDQP_OK;
}

int mpc_inputs_device(srbdqp_handle* h, const InputsArgs& c, InputsFrom from, void* stream) {
    if (const int rc = mpc_inputs_check(h, c, from)) return rc;
    if (c.B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return mpc_inputs_launch(h, c, stream ? reinterpret_cast<hipStream_t>(stream) : h->stream);
}

// the inputs on the caller's host arrays: what is present is staged around the device form
int mpc_inputs_host(srbdqp_handle* h, const InputsArgs& c) {
    if (const int rc = mpc_inputs_check(h, c, InputsFrom::Host)) return rc;
    if (c.B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)c.B, N = (size_t)h->cfg.horizon;
    InputsArgs d = c;   // the same call on device addresses
    return host_call(h, [&](HostIo& io) {
        d.x0 = io.in<double>(c.x0, b * 13 * 8); d.feet = io.in<double>(c.feet, b * 12 * 8); d.stamp = io.in<double>(c.stamp, b * 8);
        d.vel = io.in<double>(c.vel, b * ((c.flavour & kSteered) ? 3 : 2) * 8); d.standing = io.in<uint8_t>(c.standing, b);
        d.x_ref = io.out<double>(c.x_ref, b * N * 13 * 8); d.foot = io.out<double>(c.foot, b * N * 12 * 8); d.contact = io.out<uint8_t>(c.contact, b * N * 4);
        d.pcom = io.out<double>(c.pcom, b * N * 3 * 8); d.landing = io.out<double>(c.landing, b * 3 * 8); d.landing_yaw = io.out<double>(c.landing_yaw, b * 8);
        if (c.flavour & kTracked) d.pose = io.add<double>(c.pose, c.pose, b * 3 * 8, false);
        if (c.flavour & kPreview) d.previewed = io.out<uint8_t>(c.previewed, b * N * 4);
    }, [&](hipStream_t st) { return mpc_inputs_device(h, d, InputsFrom::Staged, st); });
}

// ---- the K-step loop: one argument record, one check, one loop, one host path for the eight srbdqp_fleet_rollout_* entry points ----
// what a roll-out does beside mpc_inputs -> solve -> fleet_advance (the flavour bits above): an observer behind every plant step (section 19), steered inputs
// and footholds (section 20).  (The ground is the handle's: a terrain set makes any of them a terrain roll-out, section 18)

// the arguments of a roll-out, as its entry point got them: device addresses, or the caller's host arrays (fleet_rollout_host)
struct RolloutArgs {
    int64_t B; int32_t T;
    double *x, *feet, *stamp;
    const double* v_ref;               // [B][2], null in a steered roll-out
    const double* command;             // [B][3] held (command_steps 1) or [T][B][3] (command_steps T); null unless steered
    int32_t command_steps;
    const uint8_t* standing; const double* push; const srbdqp_fleet_settings* cfg; uint8_t* alive;
    double *x_log, *u0_log, *feet_log; int32_t *status_log, *iters_log;
    const srbdqp_observer_settings* obs; double *w_est, *w_log;   // read in an observed roll-out only
    unsigned flavour;                  // kSteered: srbdqp_fleet_rollout_steered_*, which with obs is kObserved too; kObserved: ..._observed_*
    const char* fn;                    // the roll-out the call becomes, for error texts: srbdqp_fleet_rollout or srbdqp_fleet_rollout_observed
    const srbdqp_track_settings* trk; double *pose, *pose_log;    // read in a tracked roll-out only (kTracked, beside kSteered)
    const srbdqp_preview_settings* prv;                           // read in a previewed roll-out only (kPreview, beside kSteered)
};

// the horizon buffers of a roll-out of this flavour (kObserved | kSteered), at B robots, carved from one allocation of the handle's.  What a flavour has
// asked for once stays carved
int ensure_fleet_buffers(srbdqp_handle* h, size_t B, unsigned flavour) {
    auto& f = h->fleet;
    const bool terrain = h->terrain.map.h != nullptr;
    if (f.mem && f.B >= B && (!terrain || f.normals) && (!(flavour & kObserved) || f.ew) && (!(flavour & kSteered) || f.landing_yaw) &&
        (!(flavour & kPreview) || f.previewed)) return SRBDQP_OK;
    f.flavour |= flavour;
    const bool observed = f.flavour & kObserved, steered = f.flavour & kSteered, preview = f.flavour & kPreview;
    const size_t N = (size_t)h->cfg.horizon;
    auto carve = [&](char* base) {
        Carver c(base);
        f.x_ref = c.take<double>(B * N * 13); f.foot = c.take<double>(B * N * 12); f.pcom = c.take<double>(B * N * 3); f.landing = c.take<double>(B * 3);
        f.u = c.take<double>(B * N * 12); f.x_out = c.take<double>(B * (N + 1) * 13); f.contact = c.take<uint8_t>(B * N * 4);
        f.status = c.take<int32_t>(B); f.iters = c.take<int32_t>(B);
        f.normals = terrain ? c.take<double>(B * N * 12) : nullptr;
        f.ew = observed ? c.take<double>(B * N * 6) : nullptr;
        f.ring_x = observed ? c.take<double>(2 * B * 13) : nullptr; f.ring_feet = observed ? c.take<double>(2 * B * 12) : nullptr;
        f.landing_yaw = steered ? c.take<double>(B) : nullptr;
        f.previewed = preview ? c.take<uint8_t>(B * N * 4) : nullptr;
        return c.off;
    };
    const size_t want = carve(nullptr);
    if (f.mem) {   // a smaller set may still be in use by an earlier roll-out, on any stream
        if (const int rc = quiesce_all_streams(h)) return rc;
        HIP_TRY(h, hipDeviceSynchronize());
    }
    f.B = 0;
    size_t cap = f.mem ? f.bytes : 0;
    if (const int rc = grow(h, f.mem, cap, want, nullptr, "hipMalloc roll-out buffers")) { f.bytes = cap; return rc; }
    f.bytes = cap;
    carve(f.mem);
    f.B = B;
    return SRBDQP_OK;
}

// ---- the momentum observer and the roll-out that reads it (include/srbdqp_cascade.h; the kernel: srbdqp_observer.hpp) ----
// what is wrong with an observer's settings (null: nothing).  The bounds keep every value an observer writes inside the rule of srbdqp_set_external_wrench
const char* observer_settings_fault(const srbdqp_observer_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_observer_settings)) return "struct_size is not sizeof(srbdqp_observer_settings)";
    if (!(s->gain > 0.0 && s->gain <= 1.0)) return "gain must lie in (0, 1]";
    if (!(s->horizon_decay >= 0.0 && s->horizon_decay <= 1.0)) return "horizon_decay must lie in [0, 1]";
    for (const double v : {s->torque_max, s->force_max})
        if (!std::isfinite(v) || !(v > 0.0) || v > SRBDQP_EXT_WRENCH_MAX) return "torque_max and force_max must be finite, positive and at most SRBDQP_EXT_WRENCH_MAX (1e6)";
    return nullptr;
}

// one launch of the observer; the arguments have been checked.  fill: no measurement -- ew from w_est as it stands (the wrench of a roll-out's first solve)
int wrench_observer_launch(srbdqp_handle* h, int64_t B, const double* x_prev, const double* x_next, const double* feet_prev, const double* u0, int64_t u0_stride,
                           const uint8_t* alive, const srbdqp_observer_settings* cfg, double* w_est, double* ew, double* w_log, bool fill, hipStream_t st) {
    srbdqp::ObserverArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x_prev = x_prev; a.x_next = x_next; a.feet = feet_prev; a.u0 = u0; a.u0_stride = (long long)u0_stride; a.alive = alive;
    a.robots = reinterpret_cast<const double*>(h->robots.dev);   // robot b's own mass and inertia, as the plant step reads them
    a.w_est = w_est; a.ew = ew; a.w_log = w_log;
    a.mass = h->cfg.mass;
    for (int i = 0; i < 3; ++i) a.inertia[i] = h->cfg.inertia[i];
    a.dt = h->cfg.dt; a.gain = cfg->gain; a.decay = cfg->horizon_decay; a.torque_max = cfg->torque_max; a.force_max = cfg->force_max;
    a.N = (int32_t)h->cfg.horizon; a.fill_only = fill ? 1 : 0;
    a.B = (long long)B;
    HIP_TRY(h, srbdqp::launch_wrench_observer(a, st));
    h->kname = "wrench_observer_f64";
    return SRBDQP_OK;
}

int wrench_observer_check(srbdqp_handle* h, int64_t B, const void* x_prev, const void* x_next, const void* feet_prev, const void* u0, int64_t u0_stride,
                          const srbdqp_observer_settings* cfg, const void* w_est) {
    if (const int rc = arrays_check(h, B >= 0 && B <= 0x7fffffffLL, B, !x_prev || !x_next || !feet_prev || !u0 || !w_est)) return rc;
    if (u0_stride < 12) { h->err = "srbdqp_wrench_observer: u0_stride must be at least 12 doubles"; return SRBDQP_E_INVALID; }
    if (const char* why = observer_settings_fault(cfg)) { h->err = std::string("invalid srbdqp_observer_settings: ") + why; return SRBDQP_E_INVALID; }
    return covers<RobotsIn>(h, B, "srbdqp_wrench_observer: ", " robots with ", false, false);
}

// May this handle run this roll-out?  host: the arrays are the caller's host arrays.  In order:
//  * steered: the command's own rules, which need no handle and come first (host: every entry of the command must be finite);
//  * the arguments: sizes, arrays, w_est in an observed roll-out, the two settings;
//  * the handle's state, for the roll-out the call becomes.  Observed: what check_staged_side<ExtWrenchIn> refuses -- in the refusal table's words -- except robot records and
//    weights, which the wrench's batch kernel reads beside the wrench; then a terrain.  On a terrain: the solves read the normals of the call, and no instantiation
//    reads those beside another side input, on a live horizon, with rank-aware steps or at N = 24 -- what the staged normals calls refuse, in the refusal table's
//    words.  Plain: the plant is flat ground and knows no wrench but the push -- a handle whose QPs are told otherwise would roll out against another robot
constexpr unsigned kFormsObservedRollout = bit(Form::Robots) | bit(Form::Weights);
int fleet_rollout_check(srbdqp_handle* h, const RolloutArgs& a, bool host) {
    const bool preview = a.flavour & kPreview;
    if (a.flavour & kSteered) {
        const bool tracked = a.flavour & kTracked;
        const char* const who = preview ? "srbdqp_fleet_rollout_previewed" : tracked ? "srbdqp_fleet_rollout_tracked" : "srbdqp_fleet_rollout_steered";
        if (!a.command) return steer_refuse(h, std::string(who) + ": command is NULL ([B][3] held over the call, or [T][B][3] with command_steps = T)");
        if (a.command_steps != 1 && a.command_steps != a.T) return steer_refuse(h, std::string(who) + ": command_steps must be 1 (one command held) or T (a row per step)");
        if (preview) if (const char* why = preview_settings_fault(a.prv)) return steer_refuse(h, std::string(who) + ": invalid srbdqp_preview_settings: " + why);
        // tracked: the settings and the pose, and on host arrays a pose and a command that are finite
        if (tracked) { if (const int rc = track_check(h, who, a.B, a.trk, a.pose, a.T >= 1 ? a.command : nullptr, (size_t)a.command_steps, host)) return rc; }
        else if (host && a.B >= 1 && a.B <= 0x7fffffffLL && a.T >= 1) {
            const long long i = steer_non_finite(a.command, (size_t)a.command_steps * (size_t)a.B * 3);
            if (i >= 0) return steer_refuse(h, std::string(who) + ": the command of robot " + std::to_string((i / 3) % a.B) + " at row " + std::to_string(i / (3 * a.B)) + " is not finite");
        }
    }
    if (!h) return SRBDQP_E_INVALID;
    const std::string fn = a.fn;
    const bool observed = a.flavour & kObserved;
    if (a.B < 1 || a.T < 1 || a.B > 0x7fffffffLL) { h->err = fn + ": B and T must be at least 1 (B at most 2^31 - 1)"; return SRBDQP_E_INVALID; }
    if (!a.x || !a.feet || !a.stamp || !(a.v_ref || a.command)) { h->err = "null input/output pointer"; return SRBDQP_E_INVALID; }
    if (observed && !a.w_est) { h->err = fn + ": w_est is NULL (the estimate goes in and out: zeros start from no push)"; return SRBDQP_E_INVALID; }
    if (const char* why = fleet_settings_fault(a.cfg)) { h->err = std::string("invalid srbdqp_fleet_settings: ") + why; return SRBDQP_E_INVALID; }
    if (preview && a.prv->foot_half_length != a.cfg->foot_half_length) {   // the MPC would preview another foot than the plant puts down
        h->err = "srbdqp_fleet_rollout_previewed: srbdqp_preview_settings.foot_half_length differs from srbdqp_fleet_settings.foot_half_length: the footholds previewed would not be the ones the plant puts down";
        return SRBDQP_E_INVALID;
    }
    if (observed) {
        const char* const in = " -- in an observed roll-out";
        if (const char* why = observer_settings_fault(a.obs)) { h->err = std::string("invalid srbdqp_observer_settings: ") + why; return SRBDQP_E_INVALID; }
        if (const unsigned other = state_of(h) & ~kFormsObservedRollout) { const int rc = refuse(h, refusal_form(other), a.fn); h->err += in; return rc; }
        if (h->cfg.horizon > row(Form::ExtWrench).max_horizon) { h->err = fn + ": " + ExtWrenchIn::n24(a.fn) + in; return SRBDQP_E_INVALID; }
        if (!general_allowed(h->cfg)) {
            h->err = fn + ": " + row(Form::ExtWrench).noun + " is read by the general kernel only: srbdqp_config.kernel must be SRBDQP_KERNEL_AUTO or SRBDQP_KERNEL_WRENCH" + in;
            return SRBDQP_E_INVALID;
        }
        if (h->terrain.map.h) {
            h->err = fn + ": refused while a terrain is set (srbdqp_set_terrain): no instantiation reads contact normals beside a wrench (DESIGN.md section 13) -- srbdqp_set_terrain(h, NULL, NULL) goes back to flat ground";
            return SRBDQP_E_INVALID;
        }
    } else if (h->terrain.map.h) {
        if (const int rc = check_staged_side<NormalsIn>(h, a.fn)) { h->err += " -- while a terrain is set (srbdqp_set_terrain)"; return rc; }
        return SRBDQP_OK;
    } else {
        if (h->ext.dev) { h->err = fn + ": the handle has an external wrench set (srbdqp_set_external_wrench): the plant does not know it -- clear it, and pass the roll-out its push"; return SRBDQP_E_INVALID; }
        if (h->normals.dev) { h->err = fn + ": the handle has contact normals set (srbdqp_set_contact_normals): the plant stands on flat ground -- clear them"; return SRBDQP_E_INVALID; }
    }
    return variant_check_batch(h, (int32_t)a.B);   // (records and weights for every robot)
}

// ---- the ground under the fleet (include/srbdqp_cascade.h; the sample and the kernels: srbdqp_terrain.hpp) ----
int terrain_sample_check(srbdqp_handle* h, int64_t M, const void* xy, const void* z) {
    if (!h) return SRBDQP_E_INVALID;
    if (!h->terrain.map.h) { h->err = "srbdqp_terrain_sample: no terrain is set (srbdqp_set_terrain)"; return SRBDQP_E_INVALID; }
    return arrays_check(h, M >= 0, M, !xy || !z);
}

int terrain_inputs_check(srbdqp_handle* h, int64_t B, const void* feet, const void* x_ref, const void* normals) {
    if (!h) return SRBDQP_E_INVALID;
    if (!h->terrain.map.h) { h->err = "srbdqp_terrain_inputs: no terrain is set (srbdqp_set_terrain)"; return SRBDQP_E_INVALID; }
    return arrays_check(h, B >= 0 && B <= 0x7fffffffLL, B, !feet || !x_ref || !normals);
}

// one launch of the terrain's inputs; the arguments have been checked
int terrain_inputs_launch(srbdqp_handle* h, int64_t B, const double* feet, double* x_ref, double* normals, hipStream_t st) {
    srbdqp::TerrainInputsArgs a{h->terrain.map, feet, x_ref, normals, (int32_t)h->cfg.horizon, (long long)B};
    HIP_TRY(h, srbdqp::launch_terrain_inputs(a, st));
    h->kname = "terrain_inputs_f64";
    return SRBDQP_OK;
}

// ... under footholds that differ from step to step (section 22): foot's previewed points get their heights
int terrain_inputs_previewed_launch(srbdqp_handle* h, int64_t B, double* foot, const uint8_t* previewed, double* x_ref, double* normals, hipStream_t st) {
    srbdqp::TerrainPreviewArgs a{h->terrain.map, foot, previewed, x_ref, normals, (int32_t)h->cfg.horizon, (long long)B};
    HIP_TRY(h, srbdqp::launch_terrain_inputs_previewed(a, st));
    h->kname = "terrain_inputs_previewed_f64";
    return SRBDQP_OK;
}

}  // namespace

extern "C" {

// ---- the ground under the fleet (include/srbdqp_cascade.h; the sample and the kernels: srbdqp_terrain.hpp) ----
int srbdqp_set_terrain(srbdqp_handle* h, const srbdqp_terrain* t, const double* heights) {
    if (!h) return SRBDQP_E_INVALID;
    auto& tr = h->terrain;
    const bool clear = !t || !heights;
    if (!clear) {
        auto bad = [&](const std::string& why) { h->err = "srbdqp_set_terrain: " + why + "; the previous setting is kept"; return SRBDQP_E_INVALID; };
        if (t->struct_size != (int32_t)sizeof(srbdqp_terrain)) return bad("struct_size is not sizeof(srbdqp_terrain)");
        if (t->nx < 2 || t->ny < 2 || (long long)t->nx * (long long)t->ny > (1LL << 24)) return bad("nx and ny must be at least 2 and nx ny at most 2^24");
        if (!std::isfinite(t->cell) || !(t->cell > 0.0)) return bad("cell must be finite and positive");
        if (!std::isfinite(t->x0) || !std::isfinite(t->y0)) return bad("the origin (x0, y0) must be finite");
        const size_t nx = (size_t)t->nx, ny = (size_t)t->ny;
        const double step = 1.2 * t->cell;
        auto node = [](size_t i, size_t j) { return "(" + std::to_string(i) + ", " + std::to_string(j) + ")"; };
        for (size_t j = 0; j < ny; ++j)
            for (size_t i = 0; i < nx; ++i)
                if (!std::isfinite(heights[j * nx + i])) return bad("the height of node " + node(i, j) + " is not finite");
        for (size_t j = 0; j < ny; ++j)
            for (size_t i = 0; i < nx; ++i) {
                const double v = heights[j * nx + i];
                if (i + 1 < nx && std::fabs(heights[j * nx + i + 1] - v) > step) return bad("the heights of nodes " + node(i, j) + " and " + node(i + 1, j) + " differ by more than 1.2 cell (a normal would leave n_z >= 0.5)");
                if (j + 1 < ny && std::fabs(heights[(j + 1) * nx + i] - v) > step) return bad("the heights of nodes " + node(i, j) + " and " + node(i, j + 1) + " differ by more than 1.2 cell (a normal would leave n_z >= 0.5)");
            }
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (tr.map.h) {   // a launch on any stream may still read the map that is set
        if (const int rc = quiesce_all_streams(h)) return rc;
        HIP_TRY(h, hipDeviceSynchronize());
    }
    tr.map = srbdqp::TerrainMap{};
    if (clear) return SRBDQP_OK;
    const size_t count = (size_t)t->nx * (size_t)t->ny;
    if (const int rc = grow(h, tr.own, tr.cap, count, nullptr, "hipMalloc terrain")) return rc;
    HIP_TRY(h, hipMemcpy(tr.own, heights, count * sizeof(double), hipMemcpyHostToDevice));
    tr.map.h = tr.own; tr.map.nx = t->nx; tr.map.ny = t->ny; tr.map.x0 = t->x0; tr.map.y0 = t->y0; tr.map.cell = t->cell;
    return SRBDQP_OK;
}

int srbdqp_terrain_sample_device_f64(srbdqp_handle* h, int64_t M, const double* xy, double* z, double* normal, void* stream) {
    if (const int rc = terrain_sample_check(h, M, xy, z)) return rc;
    if (M == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    srbdqp::TerrainSampleArgs a{h->terrain.map, xy, z, normal, (long long)M};
    HIP_TRY(h, srbdqp::launch_terrain_sample(a, stream ? reinterpret_cast<hipStream_t>(stream) : h->stream));
    h->kname = "terrain_sample_f64";
    return SRBDQP_OK;
}

int srbdqp_terrain_sample_f64(srbdqp_handle* h, int64_t M, const double* xy, double* z, double* normal) {
    if (const int rc = terrain_sample_check(h, M, xy, z)) return rc;
    if (M == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t m = (size_t)M;
    double *dxy, *dz, *dn;
    return host_call(h, [&](HostIo& io) {
        dxy = io.in<double>(xy, m * 2 * 8); dz = io.out<double>(z, m * 8); dn = io.out<double>(normal, m * 3 * 8);
    }, [&](hipStream_t st) { return srbdqp_terrain_sample_device_f64(h, M, dxy, dz, dn, st); });
}

int srbdqp_terrain_inputs_device_f64(srbdqp_handle* h, int64_t B, const double* feet, double* x_ref, double* normals, void* stream) {
    if (const int rc = terrain_inputs_check(h, B, feet, x_ref, normals)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return terrain_inputs_launch(h, B, feet, x_ref, normals, stream ? reinterpret_cast<hipStream_t>(stream) : h->stream);
}

int srbdqp_terrain_inputs_f64(srbdqp_handle* h, int64_t B, const double* feet, double* x_ref, double* normals) {
    if (const int rc = terrain_inputs_check(h, B, feet, x_ref, normals)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)B, N = (size_t)h->cfg.horizon;
    double *dfe, *dxr, *dcn;
    return host_call(h, [&](HostIo& io) {
        dfe = io.in<double>(feet, b * 12 * 8); dxr = io.add<double>(x_ref, x_ref, b * N * 13 * 8, false); dcn = io.out<double>(normals, b * N * 12 * 8);
    }, [&](hipStream_t st) { return srbdqp_terrain_inputs_device_f64(h, B, dfe, dxr, dcn, st); });
}

int srbdqp_terrain_inputs_previewed_device_f64(srbdqp_handle* h, int64_t B, double* foot, const uint8_t* previewed, double* x_ref, double* normals, void* stream) {
    if (const int rc = terrain_inputs_check(h, B, foot, x_ref, normals)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return terrain_inputs_previewed_launch(h, B, foot, previewed, x_ref, normals, stream ? reinterpret_cast<hipStream_t>(stream) : h->stream);
}

int srbdqp_terrain_inputs_previewed_f64(srbdqp_handle* h, int64_t B, double* foot, const uint8_t* previewed, double* x_ref, double* normals) {
    if (const int rc = terrain_inputs_check(h, B, foot, x_ref, normals)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)B, N = (size_t)h->cfg.horizon;
    double *dfo, *dxr, *dcn;
    uint8_t* dpv;
    return host_call(h, [&](HostIo& io) {
        dfo = io.add<double>(foot, foot, b * N * 12 * 8, false); dpv = io.in<uint8_t>(previewed, b * N * 4);
        dxr = io.add<double>(x_ref, x_ref, b * N * 13 * 8, false); dcn = io.out<double>(normals, b * N * 12 * 8);
    }, [&](hipStream_t st) { return srbdqp_terrain_inputs_previewed_device_f64(h, B, dfo, dpv, dxr, dcn, st); });
}

int srbdqp_fleet_default_settings(srbdqp_fleet_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_fleet_settings)) return SRBDQP_E_INVALID;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = (int32_t)sizeof(srbdqp_fleet_settings);
    s->substeps = 10; s->foot_half_length = 0.085; s->z_min = 0.3; s->tilt_max = 1.0;
    s->gait.struct_size = (int32_t)sizeof(srbdqp_gait);
    s->gait.period_steps = 6; s->gait.double_support_steps = 1; s->gait.hip_offset_y = 0.0645;
    return SRBDQP_OK;
}

}  // extern "C"

namespace {
// the K-step loop; fleet_rollout_check has passed, so a.obs says whether the roll-out is observed (flat ground: the solves read the handle's wrench buffer, which
// the observer behind every plant step writes) and a.command whether it is steered.  Neither: the roll-out of section 17 / 18
int fleet_rollout_run(srbdqp_handle* h, const RolloutArgs& a, void* stream) {
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int64_t B = a.B;
    const size_t b = (size_t)B, N = (size_t)h->cfg.horizon;
    if (const int rc = ensure_fleet_buffers(h, b, a.flavour)) return rc;
    const auto& f = h->fleet;
    const bool terrain = h->terrain.map.h != nullptr;
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
    if (a.x_log) HIP_TRY(h, hipMemcpyAsync(a.x_log, a.x, b * 13 * 8, hipMemcpyDeviceToDevice, st));
    if (a.feet_log) HIP_TRY(h, hipMemcpyAsync(a.feet_log, a.feet, b * 12 * 8, hipMemcpyDeviceToDevice, st));
    if (a.obs) {
        // without the caller's logs the observer reads x_t, x_t+1 and the feet of period t from the ring, which the plant step writes as its log: entry 0 as above
        if (!a.x_log) HIP_TRY(h, hipMemcpyAsync(f.ring_x, a.x, b * 13 * 8, hipMemcpyDeviceToDevice, st));
        if (!a.feet_log) HIP_TRY(h, hipMemcpyAsync(f.ring_feet, a.feet, b * 12 * 8, hipMemcpyDeviceToDevice, st));
        // the wrench of solve 0: decay^k times the caller's estimate
        if (const int rc = wrench_observer_launch(h, B, nullptr, nullptr, nullptr, nullptr, 12, nullptr, a.obs, a.w_est, f.ew, nullptr, true, st)) return rc;
    }
    for (int32_t t = 0; t < a.T; ++t) {
        const size_t k = (size_t)t;
        // steered: row t of a schedule, or the one command held; the inputs also say how the next foot lands turned (section 20)
        // tracked: the references come from the pose the caller carries, which the inputs kernel bounds, advances and logs itself (section 21)
        const InputsArgs in{a.flavour & (kSteered | kTracked | kPreview), a.fn, B, a.x, a.feet, a.stamp,
                            a.command ? a.command + (a.command_steps == 1 ? 0 : k * b * 3) : a.v_ref, a.standing, &a.cfg->gait,
                            f.x_ref, f.foot, f.contact, f.pcom, f.landing, a.command ? f.landing_yaw : nullptr,
                            a.trk, a.pose, a.pose_log ? a.pose_log + k * b * 3 : nullptr, a.prv, (a.flavour & kPreview) ? f.previewed : nullptr};
        if (const int rc = mpc_inputs_launch(h, in, st)) return rc;
        // the ground under the footholds: the normals of this step's QPs and the height reference; previewed: under the footholds of every step (section 22)
        if (terrain) if (const int rc = (a.flavour & kPreview) ? terrain_inputs_previewed_launch(h, B, f.foot, f.previewed, f.x_ref, f.normals, st)
                                                               : terrain_inputs_launch(h, B, a.feet, f.x_ref, f.normals, st)) return rc;
        // the solve a device-buffer call makes (device_call), on a terrain with those normals as the normals of THIS call, observed with the wrench buffer as the wrench
        // of THIS call (the general kernel's _ew instantiation, which reads the handle's weights and robot records too) -- every pass of it, deferred ones on the
        // tail stream included, launches with this Call (solve_device_impl)
        Call c;
        c.use_hint = true;
        // (device memory, no host address: never inline.  fleet_rollout_check has refused an observed roll-out on a terrain)
        if (terrain) c.side = {Side::Normals, f.normals, nullptr};
        else if (a.obs) c.side = {Side::ExtWrench, f.ew, nullptr};
        c.plan = plan_solve(h, c, (int)B, maxs_or(h->cfg, 4));
        if (const int rc = solve_device_impl(h, c, (int32_t)B, a.x, f.x_ref, f.foot, f.contact, f.pcom, nullptr, nullptr, f.u, f.x_out, nullptr, f.status, f.iters, st))
            return rc;
        if (h->cfg.flags & SRBDQP_FLAG_DEFER_TAIL) if (const int rc = srbdqp_flush(h, st)) return rc;   // the plant needs complete forces
        FleetLogs lg;
        lg.x = a.x_log ? a.x_log + (k + 1) * b * 13 : nullptr; lg.feet = a.feet_log ? a.feet_log + (k + 1) * b * 12 : nullptr; lg.u0 = a.u0_log ? a.u0_log + k * b * 12 : nullptr;
        lg.status = f.status; lg.iters = f.iters;
        lg.status_log = a.status_log ? a.status_log + k * b : nullptr; lg.iters_log = a.iters_log ? a.iters_log + k * b : nullptr;
        // (observed, without the caller's logs: the state and the feet behind period t go to the ring's other slot)
        const double *x_prev = nullptr, *feet_prev = nullptr;
        if (a.obs) {
            x_prev = a.x_log ? a.x_log + k * b * 13 : f.ring_x + (k & 1) * b * 13;
            feet_prev = a.feet_log ? a.feet_log + k * b * 12 : f.ring_feet + (k & 1) * b * 12;
            if (!a.x_log) lg.x = f.ring_x + ((k + 1) & 1) * b * 13;
            if (!a.feet_log) lg.feet = f.ring_feet + ((k + 1) & 1) * b * 12;
        }
        if (const int rc = fleet_advance_launch(h, B, a.x, a.feet, a.stamp, f.u, (int64_t)(12 * N), f.landing, a.command ? f.landing_yaw : nullptr, a.standing,
                                                a.push ? a.push + k * b * 6 : nullptr, a.alive, a.cfg, lg, st))
            return rc;
        // the observer over period t: the estimate behind it, and the wrench solve t + 1 reads
        if (a.obs) if (const int rc = wrench_observer_launch(h, B, x_prev, lg.x, feet_prev, f.u, (int64_t)(12 * N), a.alive, a.obs, a.w_est, f.ew, a.w_log ? a.w_log + k * b * 6 : nullptr, false, st))
            return rc;
    }
    return SRBDQP_OK;
}

int fleet_rollout_device(srbdqp_handle* h, const RolloutArgs& a, void* stream) {
    if (const int rc = fleet_rollout_check(h, a, false)) return rc;
    return fleet_rollout_run(h, a, stream);
}

// the roll-out on the caller's host arrays: what is present is staged around the loop
int fleet_rollout_host(srbdqp_handle* h, RolloutArgs a) {
    if (const int rc = fleet_rollout_check(h, a, true)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)a.B, steps = (size_t)a.T;
    RolloutArgs d = a;   // the same call on device addresses
    return host_call(h, [&](HostIo& io) {
        d.x = io.add<double>(a.x, a.x, b * 13 * 8, false); d.feet = io.add<double>(a.feet, a.feet, b * 12 * 8, false); d.stamp = io.add<double>(a.stamp, a.stamp, b * 8, false);
        d.v_ref = io.in<double>(a.v_ref, b * 2 * 8); d.command = io.in<double>(a.command, (size_t)a.command_steps * b * 3 * 8);
        d.standing = io.in<uint8_t>(a.standing, b); d.push = io.in<double>(a.push, steps * b * 6 * 8);
        d.alive = a.alive ? io.add<uint8_t>(a.alive, a.alive, b, false) : nullptr;
        d.x_log = io.out<double>(a.x_log, (steps + 1) * b * 13 * 8); d.u0_log = io.out<double>(a.u0_log, steps * b * 12 * 8); d.feet_log = io.out<double>(a.feet_log, (steps + 1) * b * 12 * 8);
        d.status_log = io.out<int32_t>(a.status_log, steps * b * 4); d.iters_log = io.out<int32_t>(a.iters_log, steps * b * 4);
        if (a.obs) { d.w_est = io.add<double>(a.w_est, a.w_est, b * 6 * 8, false); d.w_log = io.out<double>(a.w_log, steps * b * 6 * 8); }
        if (a.pose) { d.pose = io.add<double>(a.pose, a.pose, b * 3 * 8, false); d.pose_log = io.out<double>(a.pose_log, steps * b * 3 * 8); }
    }, [&](hipStream_t st) { return fleet_rollout_run(h, d, st); });
}
}  // namespace

extern "C" {

int srbdqp_fleet_advance_device_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                                    const double* landing, const uint8_t* standing, const double* push, uint8_t* alive,
                                    const srbdqp_fleet_settings* cfg, void* stream) {
    return fleet_advance_device(h, B, x, feet, stamp, u0, u0_stride, landing, nullptr, false, standing, push, alive, cfg, stream);
}

int srbdqp_fleet_advance_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                             const double* landing, const uint8_t* standing, const double* push, uint8_t* alive,
                             const srbdqp_fleet_settings* cfg) {
    return fleet_advance_host(h, B, x, feet, stamp, u0, u0_stride, landing, nullptr, false, standing, push, alive, cfg);
}

int srbdqp_fleet_advance_steered_device_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                                            const double* landing, const double* landing_yaw, const uint8_t* standing, const double* push, uint8_t* alive,
                                            const srbdqp_fleet_settings* cfg, void* stream) {
    return fleet_advance_device(h, B, x, feet, stamp, u0, u0_stride, landing, landing_yaw, true, standing, push, alive, cfg, stream);
}

int srbdqp_fleet_advance_steered_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                                     const double* landing, const double* landing_yaw, const uint8_t* standing, const double* push, uint8_t* alive,
                                     const srbdqp_fleet_settings* cfg) {
    return fleet_advance_host(h, B, x, feet, stamp, u0, u0_stride, landing, landing_yaw, true, standing, push, alive, cfg);
}

int srbdqp_mpc_inputs_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp,
                                 const double* v_ref, const uint8_t* standing, const srbdqp_gait* gait,
                                 double* x_ref, double* foot, uint8_t* contact, double* pcom, double* landing, void* stream) {
    return mpc_inputs_device(h, {0, "srbdqp_mpc_inputs", B, x0, feet, stamp, v_ref, standing, gait, x_ref, foot, contact, pcom, landing}, InputsFrom::Device, stream);
}

int srbdqp_mpc_inputs_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp,
                          const double* v_ref, const uint8_t* standing, const srbdqp_gait* gait,
                          double* x_ref, double* foot, uint8_t* contact, double* pcom, double* landing) {
    return mpc_inputs_host(h, {0, "srbdqp_mpc_inputs", B, x0, feet, stamp, v_ref, standing, gait, x_ref, foot, contact, pcom, landing});
}

int srbdqp_mpc_inputs_steered_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                         const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                         double* landing, double* landing_yaw, void* stream) {
    return mpc_inputs_device(h, {kSteered, "srbdqp_mpc_inputs_steered", B, x0, feet, stamp, command, standing, gait, x_ref, foot, contact, pcom, landing, landing_yaw},
                             InputsFrom::Device, stream);
}

int srbdqp_mpc_inputs_steered_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                  const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                  double* landing, double* landing_yaw) {
    return mpc_inputs_host(h, {kSteered, "srbdqp_mpc_inputs_steered", B, x0, feet, stamp, command, standing, gait, x_ref, foot, contact, pcom, landing, landing_yaw});
}

// ---- a fleet that follows its path (include/srbdqp_cascade.h) ----
int srbdqp_track_default_settings(srbdqp_track_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_track_settings)) return SRBDQP_E_INVALID;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = (int32_t)sizeof(srbdqp_track_settings);
    s->lead_max = 0.1; s->yaw_lead_max = 0.3;
    return SRBDQP_OK;
}

int srbdqp_mpc_inputs_tracked_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                         const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                         double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose, void* stream) {
    return mpc_inputs_device(h, {kSteered | kTracked, "srbdqp_mpc_inputs_tracked", B, x0, feet, stamp, command, standing, gait, x_ref, foot, contact, pcom, landing,
                                 landing_yaw, trk, pose}, InputsFrom::Device, stream);
}

int srbdqp_mpc_inputs_tracked_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                  const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                  double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose) {
    return mpc_inputs_host(h, {kSteered | kTracked, "srbdqp_mpc_inputs_tracked", B, x0, feet, stamp, command, standing, gait, x_ref, foot, contact, pcom, landing,
                               landing_yaw, trk, pose});
}

// ---- footholds previewed along the horizon (include/srbdqp_cascade.h) ----
int srbdqp_preview_default_settings(srbdqp_preview_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_preview_settings)) return SRBDQP_E_INVALID;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = (int32_t)sizeof(srbdqp_preview_settings);
    s->foot_half_length = 0.085;
    return SRBDQP_OK;
}

// (trk NULL: the steered form, pose ignored)
int srbdqp_mpc_inputs_previewed_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                           const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                           double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose,
                                           const srbdqp_preview_settings* prv, uint8_t* previewed, void* stream) {
    return mpc_inputs_device(h, {kSteered | kPreview | (trk ? kTracked : 0u), "srbdqp_mpc_inputs_previewed", B, x0, feet, stamp, command, standing, gait, x_ref, foot,
                                 contact, pcom, landing, landing_yaw, trk, trk ? pose : nullptr, nullptr, prv, previewed}, InputsFrom::Device, stream);
}

int srbdqp_mpc_inputs_previewed_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                    const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                    double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose,
                                    const srbdqp_preview_settings* prv, uint8_t* previewed) {
    return mpc_inputs_host(h, {kSteered | kPreview | (trk ? kTracked : 0u), "srbdqp_mpc_inputs_previewed", B, x0, feet, stamp, command, standing, gait, x_ref, foot,
                               contact, pcom, landing, landing_yaw, trk, trk ? pose : nullptr, nullptr, prv, previewed});
}

// ---- the momentum observer (include/srbdqp_cascade.h) ----
int srbdqp_observer_default_settings(srbdqp_observer_settings* s) {
    if (!s || s->struct_size != (int32_t)sizeof(srbdqp_observer_settings)) return SRBDQP_E_INVALID;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = (int32_t)sizeof(srbdqp_observer_settings);
    s->gain = 0.5; s->horizon_decay = 1.0; s->torque_max = 50.0; s->force_max = 200.0;
    return SRBDQP_OK;
}

int srbdqp_wrench_observer_device_f64(srbdqp_handle* h, int64_t B, const double* x_prev, const double* x_next, const double* feet_prev, const double* u0,
                                      int64_t u0_stride, const uint8_t* alive, const srbdqp_observer_settings* cfg, double* w_est, double* ew_out,
                                      void* stream) {
    if (const int rc = wrench_observer_check(h, B, x_prev, x_next, feet_prev, u0, u0_stride, cfg, w_est)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : h->stream;
    return wrench_observer_launch(h, B, x_prev, x_next, feet_prev, u0, u0_stride, alive, cfg, w_est, ew_out, nullptr, false, st);
}

int srbdqp_wrench_observer_f64(srbdqp_handle* h, int64_t B, const double* x_prev, const double* x_next, const double* feet_prev, const double* u0,
                               int64_t u0_stride, const uint8_t* alive, const srbdqp_observer_settings* cfg, double* w_est, double* ew_out) {
    if (const int rc = wrench_observer_check(h, B, x_prev, x_next, feet_prev, u0, u0_stride, cfg, w_est)) return rc;
    if (B == 0) return SRBDQP_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t b = (size_t)B, N = (size_t)h->cfg.horizon;
    double *dx0, *dx1, *dfe, *du, *dw, *dew;
    uint8_t* dal;
    return host_call(h, [&](HostIo& io) {
        dx0 = io.in<double>(x_prev, b * 13 * 8); dx1 = io.in<double>(x_next, b * 13 * 8); dfe = io.in<double>(feet_prev, b * 12 * 8);
        du = io.in<double>(u0, ((b - 1) * (size_t)u0_stride + 12) * 8); dal = io.in<uint8_t>(alive, b);
        dw = io.add<double>(w_est, w_est, b * 6 * 8, false); dew = io.out<double>(ew_out, b * N * 6 * 8);
    }, [&](hipStream_t st) { return srbdqp_wrench_observer_device_f64(h, B, dx0, dx1, dfe, du, u0_stride, dal, cfg, dw, dew, st); });
}

// ---- the eight roll-outs: each fills the record (RolloutArgs) and calls through ----
int srbdqp_fleet_rollout_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                                    const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                    double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log, void* stream) {
    return fleet_rollout_device(h, {B, T, x, feet, stamp, v_ref, nullptr, 1, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                    nullptr, nullptr, nullptr, 0, "srbdqp_fleet_rollout"}, stream);
}

int srbdqp_fleet_rollout_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                             const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                             double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log) {
    return fleet_rollout_host(h, {B, T, x, feet, stamp, v_ref, nullptr, 1, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                  nullptr, nullptr, nullptr, 0, "srbdqp_fleet_rollout"});
}

int srbdqp_fleet_rollout_observed_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                                             const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                             double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                             const srbdqp_observer_settings* obs, double* w_est, double* w_log, void* stream) {
    return fleet_rollout_device(h, {B, T, x, feet, stamp, v_ref, nullptr, 1, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                    obs, w_est, w_log, kObserved, "srbdqp_fleet_rollout_observed"}, stream);
}

int srbdqp_fleet_rollout_observed_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                                      const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                      double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                      const srbdqp_observer_settings* obs, double* w_est, double* w_log) {
    return fleet_rollout_host(h, {B, T, x, feet, stamp, v_ref, nullptr, 1, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                  obs, w_est, w_log, kObserved, "srbdqp_fleet_rollout_observed"});
}

// (a steered call with an observer is refused in the observed roll-out's words, one without in the plain one's)
int srbdqp_fleet_rollout_steered_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                            int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                            double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                            const srbdqp_observer_settings* obs, double* w_est, double* w_log, void* stream) {
    return fleet_rollout_device(h, {B, T, x, feet, stamp, nullptr, command, command_steps, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                    obs, w_est, w_log, kSteered | (obs ? kObserved : 0u), obs ? "srbdqp_fleet_rollout_observed" : "srbdqp_fleet_rollout"}, stream);
}

int srbdqp_fleet_rollout_steered_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                     int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                     double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                     const srbdqp_observer_settings* obs, double* w_est, double* w_log) {
    return fleet_rollout_host(h, {B, T, x, feet, stamp, nullptr, command, command_steps, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                  obs, w_est, w_log, kSteered | (obs ? kObserved : 0u), obs ? "srbdqp_fleet_rollout_observed" : "srbdqp_fleet_rollout"});
}

// (the steered roll-out with the tracked inputs call: refused as the roll-out it becomes is, after the pose's and the settings' own rules)
int srbdqp_fleet_rollout_tracked_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                            int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                            double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                            const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                            const srbdqp_track_settings* trk, double* pose, double* pose_log, void* stream) {
    return fleet_rollout_device(h, {B, T, x, feet, stamp, nullptr, command, command_steps, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                    obs, w_est, w_log, kTracked | kSteered | (obs ? kObserved : 0u), obs ? "srbdqp_fleet_rollout_observed" : "srbdqp_fleet_rollout",
                                    trk, pose, pose_log}, stream);
}

int srbdqp_fleet_rollout_tracked_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                     int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                     double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                     const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                     const srbdqp_track_settings* trk, double* pose, double* pose_log) {
    return fleet_rollout_host(h, {B, T, x, feet, stamp, nullptr, command, command_steps, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                  obs, w_est, w_log, kTracked | kSteered | (obs ? kObserved : 0u), obs ? "srbdqp_fleet_rollout_observed" : "srbdqp_fleet_rollout",
                                  trk, pose, pose_log});
}

// (the steered roll-out, tracked where trk is given, with the previewed inputs call -- and on a terrain the previewed terrain inputs)
int srbdqp_fleet_rollout_previewed_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                              int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                              double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                              const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                              const srbdqp_track_settings* trk, double* pose, double* pose_log, const srbdqp_preview_settings* prv, void* stream) {
    return fleet_rollout_device(h, {B, T, x, feet, stamp, nullptr, command, command_steps, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                    obs, w_est, w_log, kPreview | (trk ? kTracked : 0u) | kSteered | (obs ? kObserved : 0u),
                                    obs ? "srbdqp_fleet_rollout_observed" : "srbdqp_fleet_rollout", trk, trk ? pose : nullptr, trk ? pose_log : nullptr, prv}, stream);
}

int srbdqp_fleet_rollout_previewed_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                       int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                       double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                       const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                       const srbdqp_track_settings* trk, double* pose, double* pose_log, const srbdqp_preview_settings* prv) {
    return fleet_rollout_host(h, {B, T, x, feet, stamp, nullptr, command, command_steps, standing, push, cfg, alive, x_log, u0_log, feet_log, status_log, iters_log,
                                  obs, w_est, w_log, kPreview | (trk ? kTracked : 0u) | kSteered | (obs ? kObserved : 0u),
                                  obs ? "srbdqp_fleet_rollout_observed" : "srbdqp_fleet_rollout", trk, trk ? pose : nullptr, trk ? pose_log : nullptr, prv});
}

}  // extern "C"
