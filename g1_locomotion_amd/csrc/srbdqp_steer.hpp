// A fleet that steers (include/srbdqp_cascade.h, srbdqp_mpc_inputs_steered_*): the step before the QP under a command (vx, vy, wz) --
// planar velocity in the robot's heading frame and a yaw rate -- in place of a velocity fixed in the world.  The references turn with the commanded heading,
// the landing point's hip offset turns with the heading at mid-swing, psi_L, and the plant step (srbdqp_fleet.hpp) turns heel and toe by the same psi_L.
//
// steer_rotate, steer_yaw, steer_table and steer_touchdown are __host__ __device__ and need nothing of HIP: a host compiler builds them from this header alone
// (tests/test_steer_cpu.py does, against tests/steer_twin.py).  The kernel below them, srbdqp_mpc_inputs_commanded_kernel, is a template so that it is emitted
// only where it is instantiated: in srbdqp_wrench_lat_ew.hip, the library's second code object, as the fleet's kernels are; srbdqp.hip sees SteerInputsArgs,
// TrackPose and the launcher.
//
// A fleet that follows its path (srbdqp_mpc_inputs_tracked_*) takes the same references from a pose carried from step to step in place
// of the measured state: track_bound and track_advance beside steer_table (tests/test_track_cpu.py builds them alone, against tests/track_twin.py).  Its
// kernel is the same template with a TrackPose as a second argument: one text for the staging, the gait phase, the element loops and the landing point, and
// `if constexpr` around what a pose adds.
//
// A fleet that previews its footholds along the horizon (srbdqp_mpc_inputs_previewed_*): preview_lands, preview_touchdown and
// preview_foothold beside steer_landing (tests/test_preview_cpu.py builds them alone, against tests/preview_twin.py), and a PreviewFeet as the template's last
// argument, steered or tracked.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "srbdqp_gait.hpp"
#define SRBDQP_STEER_HD __host__ __device__ __forceinline__
#else
#define SRBDQP_STEER_HD inline
#endif

namespace srbdqp {

constexpr int kSteerSteps = 25;   // table entries of one robot: k = 0 ... N, N <= 24

// every product and sum below is one rounded operation, in the order written (no fused multiply-add: the twin is NumPy)

// v_w(theta) = Rz(theta) (vx, vy)
SRBDQP_STEER_HD void steer_rotate(double theta, double vx, double vy, double& wx, double& wy) {
#pragma clang fp contract(off)
    const double s = sin(theta), c = cos(theta);
    wx = c * vx - s * vy;
    wy = s * vx + c * vy;
}

// psi0 + wz (k dt) for a whole or a half step index k, as (wz k) dt
SRBDQP_STEER_HD double steer_yaw(double psi0, double wz, double k, double dt) {
#pragma clang fp contract(off)
    return psi0 + (wz * k) * dt;
}

// The reference table of one robot, entries k = 0 ... N:  p[k] = p_k, the reference position -- p_0 = (px0, py0), p_{k+1} = p_k + v_w(psi0 + wz (k + 1/2) dt) dt,
// a serial sum with the heading at the middle of the step -- and v[k] = v_w(psi0 + wz k dt).  The trip count is N whatever the command holds: a command that is
// not finite gives entries that are not numbers, nothing else.  (The kernel computes the same entries spread over a tile's threads.)
SRBDQP_STEER_HD void steer_table(double psi0, double px0, double py0, double vx, double vy, double wz, double dt, int N, double* px, double* py, double* vwx,
                                 double* vwy) {
#pragma clang fp contract(off)
    px[0] = px0; py[0] = py0;
    for (int k = 0; k <= N; ++k) {
        steer_rotate(steer_yaw(psi0, wz, (double)k, dt), vx, vy, vwx[k], vwy[k]);
        if (k < N) {
            double mx, my;
            steer_rotate(steer_yaw(psi0, wz, (double)k + 0.5, dt), vx, vy, mx, my);
            px[k + 1] = px[k] + mx * dt; py[k + 1] = py[k] + my * dt;
        }
    }
}

// A fleet that follows its path (srbdqp_mpc_inputs_tracked_*) carries a reference pose (qx, qy, th) from step to step.  track_bound keeps
// the pose within lead_max metres and yaw_lead_max radians of the measured (cx, cy, psi0): beyond, it is pulled back along the same direction.  A pose inside
// the bounds is untouched bit for bit, and every comparison is false on a NaN: a state or a pose that is not finite clamps nothing.
SRBDQP_STEER_HD void track_bound(double& qx, double& qy, double& th, double cx, double cy, double psi0, double lead_max, double yaw_lead_max) {
#pragma clang fp contract(off)
    const double dx = qx - cx, dy = qy - cy;
    const double n = sqrt(dx * dx + dy * dy);
    if (n > lead_max) {
        const double s = lead_max / n;
        qx = cx + dx * s; qy = cy + dy * s;
    }
    const double dth = th - psi0;
    if (dth > yaw_lead_max) th = psi0 + yaw_lead_max;
    else if (dth < -yaw_lead_max) th = psi0 - yaw_lead_max;
}

// ... and track_advance moves the bounded pose on by one control step: (q_1 of its table, th + (wz 1) dt).  Where one of the three is not finite the pose
// stays as track_bound left it: a bad command row costs its robot one step, not the rest of the roll-out.
SRBDQP_STEER_HD void track_advance(double& qx, double& qy, double& th, double q1x, double q1y, double wz, double dt) {
#pragma clang fp contract(off)
    const double th1 = steer_yaw(th, wz, 1.0, dt);
    if (__builtin_isfinite(q1x) && __builtin_isfinite(q1y) && __builtin_isfinite(th1)) { qx = q1x; qy = q1y; th = th1; }
}

// the touchdown of a turned foot: heel = landing - half (cos psi, sin psi), toe = landing + half (cos psi, sin psi), in the plane
SRBDQP_STEER_HD void steer_touchdown(double lx, double ly, double half, double psi, double (&heel)[2], double (&toe)[2]) {
#pragma clang fp contract(off)
    const double hx = half * cos(psi), hy = half * sin(psi);
    heel[0] = lx - hx; heel[1] = ly - hy;
    toe[0] = lx + hx; toe[1] = ly + hy;
}

// the landing point under a command: the hip offset turned by psi_L, the heading at mid-swing; vw0 = v_w(psi0); side: -1 the left foot stands, +1 the right
SRBDQP_STEER_HD void steer_landing(const double* x0, double psi_l, double side, double hip_offset_y, double half_T, double vw0x, double vw0y, double& lx, double& ly) {
#pragma clang fp contract(off)
    const double s = sin(psi_l), c = cos(psi_l), o = side * hip_offset_y;
    lx = ((x0[3] + (0.0 - s * o)) + half_T * x0[9]) + 0.03 * (x0[9] - vw0x);
    ly = ((x0[4] + c * o) + half_T * x0[10]) + 0.03 * (x0[10] - vw0y);
}

// Footholds previewed along the horizon (include/srbdqp_cascade.h, srbdqp_mpc_inputs_previewed_*): the plant's touchdown rule moved
// along the horizon.  With ph(k) = (p0 + k) mod 2 period the left foot (contacts 0, 1) is in the air for ph in [period + ds, 2 period) and lands at ph = 0, the
// right foot (contacts 2, 3) is in the air for ph in [ds, period) and lands at ph = period: closed forms of the phase, no search.  p0 < 0 (standing) and
// ds >= period (no swing) have no touchdown.  preview_lands, preview_touchdown and preview_foothold are __host__ __device__ and need nothing of HIP
// (tests/test_preview_cpu.py builds them alone, against tests/preview_twin.py).

// the foot that touches down at horizon step j: 0 none (j < 1 among it: step 0 is the present), 1 the left, 2 the right
SRBDQP_STEER_HD int preview_lands(int p0, int j, int period, int ds) {
    if (p0 < 0 || ds >= period || j < 1) return 0;
    const int ph = (p0 + j) % (2 * period);
    return ph == 0 ? 1 : (ph == period ? 2 : 0);
}

// the latest touchdown step j in [1, k] of the left (right: the right) foot, or 0 where there is none
SRBDQP_STEER_HD int preview_touchdown(int p0, int k, int period, int ds, bool right) {
    if (p0 < 0 || ds >= period) return 0;
    const int j = k - (p0 + k + (right ? period : 0)) % (2 * period);
    return j >= 1 ? j : 0;
}

// the foothold of a touchdown from the predicted state behind the step before it: heading psi, position (px, py), velocity (vx, vy), the command's velocity
// (vwx, vwy) there; side: +1 the left foot lands, -1 the right (steer_landing's side: the OTHER foot stands).  psi_l = psi + wz half_T, the landing point is
// steer_landing's, heel and toe are steer_touchdown's along psi_l
SRBDQP_STEER_HD void preview_foothold(double psi, double px, double py, double vx, double vy, double vwx, double vwy, double wz, double side, double hip_offset_y,
                                      double half_T, double half, double (&heel)[2], double (&toe)[2], double& psi_l) {
#pragma clang fp contract(off)
    double x[11] = {};
    x[3] = px; x[4] = py; x[9] = vx; x[10] = vy;
    psi_l = psi + wz * half_T;
    double lx, ly;
    steer_landing(x, psi_l, side, hip_offset_y, half_T, vwx, vwy, lx, ly);
    steer_touchdown(lx, ly, half, psi_l, heel, toe);
}

struct SteerInputsArgs {
    const double* x0;        // [B][13]
    const double* feet;      // [B][12]
    const double* stamp;     // [B]
    const double* command;   // [B][3]  (vx, vy, wz)
    const uint8_t* standing; // [B] or null
    double* x_ref;           // [B][N][13]
    double* foot;            // [B][N][12]
    uint8_t* contact;        // [B][N][4]
    double* pcom;            // [B][N][3]
    double* landing;         // [B][3] or null
    double* landing_yaw;     // [B] or null
    double com_target[3];
    double hip_offset_y, dt;
    int32_t N, period, ds;
    long long B;
};

// what a tracked call adds to the steered call's arguments: the kernel's second argument
struct TrackPose {
    double* pose;            // [B][3]  (qx, qy, th), in/out
    double* pose_log;        // [B][3] or null: a second copy of the pose written (a roll-out's pose_log[t])
    double lead_max, yaw_lead_max;
};

// what a previewed call adds: the kernel's last argument, behind the pose of a tracked call
struct PreviewFeet {
    uint8_t* previewed;      // [B][N][4] or null: 1 where foot[b][k] holds a previewed point for that contact
    double foot_half_length; // heel and toe lie this far behind and ahead of the landing point, as in the plant step
};

#if defined(__HIPCC__)
// the launch of srbdqp_mpc_inputs_commanded_kernel on st (srbdqp_wrench_lat_ew.hip); track null: the steered instantiation; live: a.N at run time
// (SRBDQP_FLAG_ANY_HORIZON); preview non-null: the previewed instantiation of either
hipError_t launch_mpc_inputs_commanded(const SteerInputsArgs& a, const TrackPose* track, bool live, hipStream_t st, const PreviewFeet* preview = nullptr);

// the argument of type T among the kernel's trailing ones
template <class T, class First, class... Rest>
__device__ __forceinline__ const T& steer_arg(const First& first, const Rest&... rest) {
    if constexpr (std::is_same<T, First>::value) return first;
    else return steer_arg<T>(rest...);
}

// srbdqp_mpc_inputs_kernel's tiling (srbdqp_cascade.hpp): a workgroup takes tiles of 32 consecutive robots, their 13 + 12 + 3 input doubles each staged in LDS
// with coalesced loads, the tile's outputs written element by element, 512 contiguous bytes per store instruction of a wave.  Between the two, the tile's
// reference table (steer_table's entries): a thread per (robot, k) takes the sines and cosines of its entry -- the heading at step k and at k + 1/2 --, then
// a thread per (robot, axis) sums the N increments in order.  The element loops read the table and take no sine.
//
// TRACK empty: the steered inputs.  One table, from the measured state: p_k and v_w(psi0 + wz k dt); a robot whose command has no planar part is referred to
// com_target.  Four [32][25] arrays, 32 KB of LDS with the staged inputs, four workgroups a CU.
//
// TRACK = TrackPose: the tracked inputs, with two tables in place of one.  The references come from the tile's poses, bounded by
// track_bound before anything reads them: q_k and v_w(th + wz k dt), moving or not.  What belongs to where the robot IS comes from the measured state as in the
// steered form, bit for bit: p_k for pcom, v_w(psi0) for the landing point.  A thread per (robot, k) takes the three sines and cosines of its entry, a thread
// per (robot, table, axis) sums the N increments in order, and a thread per robot moves its pose on (track_advance) and writes it, to pose and -- in a
// roll-out -- to the step's row of pose_log.  Six [32][25] arrays: 47 KB of LDS, three workgroups a CU.  The steered form neither holds nor
// reads what is the tracked form's alone (sq, sqx, sqy, sv0): its 32 KB are what let a fourth workgroup onto the CU.
//
// A PreviewFeet last: the previewed inputs of either form.  Behind the serial sums a thread per (robot, step k) decides from the phase
// whether a foot touches down at k; where one does it computes heel and toe (preview_foothold: three sines and cosines, from p_{k-1} of the measured table) into
// stx [32][25][4], and every thread writes the latest touchdown steps of both feet at k into sj.  The foot loop then reads sj and stx and takes no sine; the
// contact loop writes the previewed word beside the contact word.  25.6 KB + 1.6 KB of LDS more: 59 KB steered, 74 KB tracked, two workgroups a CU.
template <int NH, class... TRACK>   // NH: the horizon as a compile-time constant (NH = 0: a.N at run time)
__global__ __launch_bounds__(256) void srbdqp_mpc_inputs_commanded_kernel(SteerInputsArgs a, TRACK... track) {
#pragma clang fp contract(off)
    constexpr bool TRACKED = (std::is_same<TRACK, TrackPose>::value || ...), PREVIEW = (std::is_same<TRACK, PreviewFeet>::value || ...);
    static_assert(sizeof...(TRACK) == (TRACKED ? 1 : 0) + (PREVIEW ? 1 : 0), "at most one TrackPose, then at most one PreviewFeet");
    constexpr int R = 32, K = kSteerSteps, RT = TRACKED ? R : 1;          // RT: the rows of what only the tracked form holds
    constexpr int RP = PREVIEW ? R : 1;                                   // ... and of what only a previewed form holds
    const int N = NH > 0 ? NH : a.N;
    __shared__ double sx0[R * 13], sft[R * 12], sc[R * 3], sq[RT * 3];
    __shared__ double sqx[RT * K], sqy[RT * K], svx[R * K], svy[R * K];   // the pose's q_k; v_w(th + wz k dt) -- steered: th = psi0 --, k = 0 ... N
    __shared__ double spx[R * K], spy[R * K], sv0[RT * 2];                // the measured state's p_k; tracked: v_w(psi0) beside svx, svy
    __shared__ int sph[R];                                               // phase of step 0 in [0, 2 period), or -1 = standing
    __shared__ double stx[RP * K * 4];                                    // previewed: heel xy, toe xy of the touchdown at step k
    __shared__ uint8_t sj[RP * K * 2];                                    // previewed: the latest touchdown step of the left, the right foot at step k (0: none)
    double* const rx = TRACKED ? sqx : spx;                              // the table the references read: steered, the measured state's own
    double* const ry = TRACKED ? sqy : spy;
    const int t = threadIdx.x;
    const long long tiles = (a.B + R - 1) / R;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long b0 = tile * R;
        const int nr = (int)((a.B - b0 < R) ? (a.B - b0) : R);
        for (int i = t; i < nr * 13; i += 256) sx0[i] = a.x0[b0 * 13 + i];
        for (int i = t; i < nr * 12; i += 256) sft[i] = a.feet[b0 * 12 + i];
        for (int i = t; i < nr * 3; i += 256) {
            sc[i] = a.command[b0 * 3 + i];
            if constexpr (TRACKED) sq[i] = steer_arg<TrackPose>(track...).pose[b0 * 3 + i];
        }
        if (t < nr) {
            const bool stand = a.standing && a.standing[b0 + t];
            sph[t] = stand ? -1 : gait_phase0(a.stamp[b0 + t], a.dt, a.period);
        }
        __syncthreads();
        if constexpr (TRACKED) {
            const TrackPose& tp = steer_arg<TrackPose>(track...);
            if (t < nr) track_bound(sq[3 * t], sq[3 * t + 1], sq[3 * t + 2], sx0[13 * t + 3], sx0[13 * t + 4], sx0[13 * t + 2], tp.lead_max, tp.yaw_lead_max);
            __syncthreads();
        }
        for (int e = t; e < nr * (N + 1); e += 256) {                    // the tables' sines and cosines: entry (r, k)
            const int r = e / (N + 1), k = e - (N + 1) * r;
            const double psi0 = sx0[13 * r + 2], th = TRACKED ? sq[3 * r + 2] : psi0, vx = sc[3 * r], vy = sc[3 * r + 1], wz = sc[3 * r + 2];
            double wx, wy;
            steer_rotate(steer_yaw(th, wz, (double)k, a.dt), vx, vy, wx, wy);
            svx[K * r + k] = wx; svy[K * r + k] = wy;
            if constexpr (TRACKED) if (k == 0) {
                steer_rotate(steer_yaw(psi0, wz, 0.0, a.dt), vx, vy, wx, wy);
                sv0[2 * r] = wx; sv0[2 * r + 1] = wy;
            }
            if (k < N) {                                                 // the increments of step k, where q_{k+1} and p_{k+1} will stand
                if constexpr (TRACKED) {
                    steer_rotate(steer_yaw(th, wz, (double)k + 0.5, a.dt), vx, vy, wx, wy);
                    sqx[K * r + k + 1] = wx * a.dt; sqy[K * r + k + 1] = wy * a.dt;
                }
                steer_rotate(steer_yaw(psi0, wz, (double)k + 0.5, a.dt), vx, vy, wx, wy);
                spx[K * r + k + 1] = wx * a.dt; spy[K * r + k + 1] = wy * a.dt;
            }
        }
        __syncthreads();
        if (t < nr * (TRACKED ? 4 : 2)) {                                // the serial sums, one (robot, [table,] axis) each
            const int r = t >> (TRACKED ? 2 : 1), c = t & 1;
            const bool measured = !TRACKED || ((t >> 1) & 1);
            double* p = (measured ? (c ? spy : spx) : (c ? sqy : sqx)) + K * r;
            double acc = measured ? sx0[13 * r + 3 + c] : sq[3 * r + c];
            p[0] = acc;
            for (int k = 1; k <= N; ++k) { acc = acc + p[k]; p[k] = acc; }
        }
        __syncthreads();
        if constexpr (PREVIEW) {                                         // the touchdowns along the horizon: entry (r, k), k = 0 ... N - 1
            const PreviewFeet& pv = steer_arg<PreviewFeet>(track...);
            const double half_T = 0.5 * ((double)a.period * a.dt);
            for (int e = t; e < nr * N; e += 256) {
                const int r = e / N, k = e - N * r;
                const int lands = preview_lands(sph[r], k, a.period, a.ds);
                if (lands) {                                             // from the predicted state behind step k - 1; k - 1 = 0: the measured state itself
                    const double* x0 = sx0 + 13 * r;
                    const double vx = sc[3 * r], vy = sc[3 * r + 1], wz = sc[3 * r + 2];
                    double vwx, vwy;                                     // v_w(psi0 + wz (k - 1) dt): steered, the table's own entry
                    if constexpr (TRACKED) steer_rotate(steer_yaw(x0[2], wz, (double)(k - 1), a.dt), vx, vy, vwx, vwy);
                    else { vwx = svx[K * r + k - 1]; vwy = svy[K * r + k - 1]; }
                    const bool now = k == 1;
                    const double psi = now ? x0[2] : steer_yaw(x0[2], wz, (double)(k - 1), a.dt);
                    double heel[2], toe[2], psi_l;
                    preview_foothold(psi, spx[K * r + k - 1], spy[K * r + k - 1], now ? x0[9] : vwx, now ? x0[10] : vwy, vwx, vwy, wz, lands == 1 ? 1.0 : -1.0,
                                     a.hip_offset_y, half_T, pv.foot_half_length, heel, toe, psi_l);
                    double* o = stx + (K * r + k) * 4;
                    o[0] = heel[0]; o[1] = heel[1]; o[2] = toe[0]; o[3] = toe[1];
                }
                sj[(K * r + k) * 2] = (uint8_t)preview_touchdown(sph[r], k, a.period, a.ds, false);
                sj[(K * r + k) * 2 + 1] = (uint8_t)preview_touchdown(sph[r], k, a.period, a.ds, true);
            }
            __syncthreads();
        }
        auto flags = [&](int r, int k, bool& cl, bool& cr) { gait_flags(sph[r], k, a.period, a.ds, cl, cr); };
        double* xr = a.x_ref + b0 * (N * 13);
        for (int e = t; e < nr * N * 13; e += 256) {                     // x_ref[r][k][c], reference index k + 1
            const int row = e / 13, c = e - 13 * row, r = row / N, k = row - N * r;
            const double* x0 = sx0 + 13 * r;
            const double vx = sc[3 * r], vy = sc[3 * r + 1], wz = sc[3 * r + 2];
            const bool moving = TRACKED || (vx != 0.0) || (vy != 0.0);    // tracked: from the pose, moving or not
            double v = 0.0;
            if (c == 2) v = steer_yaw(TRACKED ? sq[3 * r + 2] : x0[2], wz, (double)(k + 1), a.dt);
            else if (c == 3) v = moving ? rx[K * r + k + 1] : a.com_target[0];
            else if (c == 4) v = moving ? ry[K * r + k + 1] : a.com_target[1];
            else if (c == 5) v = a.com_target[2];
            else if (c == 8) v = wz;
            else if (c == 9) v = svx[K * r + k + 1];
            else if (c == 10) v = svy[K * r + k + 1];
            else if (c == 12) v = x0[12];
            xr[e] = v;
        }
        double* fo = a.foot + b0 * (N * 12);
        for (int e = t; e < nr * N * 12; e += 256) {                     // foot[r][k][c]: the current contact points, repeated
            const int row = e / 12, c = e - 12 * row, r = row / N;
            if constexpr (PREVIEW) {                                     // ... or heel and toe of the foot's latest touchdown up to step k, on the ground plane
                const int k = row - N * r, i = c / 3, ax = c - 3 * i, j = sj[(K * r + k) * 2 + (i >> 1)];
                fo[e] = !j ? sft[12 * r + c] : (ax == 2 ? 0.0 : stx[(K * r + j) * 4 + 2 * (i & 1) + ax]);
            } else
                fo[e] = sft[12 * r + c];
        }
        double* pc = a.pcom + b0 * (N * 3);
        for (int e = t; e < nr * N * 3; e += 256) {                      // pcom[r][k] = (p_k, the measured height): where the robot is
            const int row = e / 3, c = e - 3 * row, r = row / N, k = row - N * r;
            pc[e] = (c == 0) ? spx[K * r + k] : (c == 1) ? spy[K * r + k] : sx0[13 * r + 5];
        }
        uint32_t* cw = reinterpret_cast<uint32_t*>(a.contact) + b0 * N;  // 4 flags per step = one aligned word
        for (int row = t; row < nr * N; row += 256) {
            const int r = row / N, k = row - N * r;
            bool cl, cr;
            flags(r, k, cl, cr);
            cw[row] = (cl ? 0x00000101u : 0u) | (cr ? 0x01010000u : 0u);
            if constexpr (PREVIEW) {
                const PreviewFeet& pv = steer_arg<PreviewFeet>(track...);
                if (pv.previewed) (reinterpret_cast<uint32_t*>(pv.previewed) + b0 * N)[row] = (sj[(K * r + k) * 2] ? 0x00000101u : 0u) | (sj[(K * r + k) * 2 + 1] ? 0x01010000u : 0u);
            }
        }
        if (t < nr) {
            const double* x0 = sx0 + 13 * t;
            const double wz = sc[3 * t + 2];
            if (a.landing || a.landing_yaw) {                            // the landing point of the foot that is (or goes next) in the air, and its heading:
                bool cl, cr;                                             // from the measured state in either form
                flags(t, 0, cl, cr);
                const double half_T = 0.5 * ((double)a.period * a.dt);
                const double psi_l = x0[2] + wz * half_T;
                if (a.landing) {
                    double lx, ly;
                    steer_landing(x0, psi_l, cl ? -1.0 : 1.0, a.hip_offset_y, half_T, TRACKED ? sv0[2 * t] : svx[K * t], TRACKED ? sv0[2 * t + 1] : svy[K * t], lx, ly);
                    a.landing[(b0 + t) * 3] = lx; a.landing[(b0 + t) * 3 + 1] = ly; a.landing[(b0 + t) * 3 + 2] = 0.0;
                }
                if (a.landing_yaw) a.landing_yaw[b0 + t] = psi_l;
            }
            if constexpr (TRACKED) {
                const TrackPose& tp = steer_arg<TrackPose>(track...);
                double qx = sq[3 * t], qy = sq[3 * t + 1], th = sq[3 * t + 2];  // the pose behind this control step
                track_advance(qx, qy, th, sqx[K * t + 1], sqy[K * t + 1], wz, a.dt);
                double* po = tp.pose + (b0 + t) * 3;
                po[0] = qx; po[1] = qy; po[2] = th;
                if (tp.pose_log) { double* pl = tp.pose_log + (b0 + t) * 3; pl[0] = qx; pl[1] = qy; pl[2] = th; }
            }
        }
        __syncthreads();
    }
}
#endif

}  // namespace srbdqp
