// One control period of a fleet between two solves (include/srbdqp_cascade.h, srbdqp_fleet_advance_*): the nonlinear single-rigid-body plant under the
// first-step forces of the solve, the gait clock, the foothold of a foot that touches down, and the robots that fell.  What tests/srbd_plant.py and the loop of
// tests/test_msgs_closed_loop.py do for one robot on the host, for B robots on the device, so that a roll-out never leaves it.
//
// The kernel is a template so that it is emitted only where it is instantiated: in srbdqp_wrench_lat_ew.hip, the library's second code object (srbdqp.hip's
// stays what it was: srbdqp_wrench_lat_ew.hpp says why that matters); srbdqp.hip sees FleetArgs and the launcher below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "srbdqp_gait.hpp"
#include "srbdqp_steer.hpp"
#include "srbdqp_terrain.hpp"

namespace srbdqp {

struct FleetArgs {
    double* x;               // [B][13]  in/out
    double* feet;            // [B][12]  in/out
    double* stamp;           // [B]      in/out
    const double* u0;        // first-step forces: robot b's twelve at u0 + b * u0_stride (u_out of a solve: stride 12 N)
    long long u0_stride;
    const double* landing;   // [B][3]   as srbdqp_mpc_inputs_kernel wrote it
    const uint8_t* standing; // [B] or null
    const double* push;      // [B][6] or null: world wrench on the body during this period, torque first
    uint8_t* alive;          // [B] or null, in/out
    const double* robots;    // per-robot records (srbdqp_robot, 8 doubles: mass, inertia[3], ...) in place of mass / inertia, or null
    // the roll-out's records of this period, each or null: the state and the feet BEHIND it, the forces it ran under, the outcome of the solve they came from
    double* x_log;           // [B][13]
    double* feet_log;        // [B][12]
    double* u0_log;          // [B][12]
    const int32_t* status;   // [B]  (read when status_log is set)
    const int32_t* iters;    // [B]
    int32_t* status_log;     // [B]
    int32_t* iters_log;      // [B]
    double mass, inertia[3];
    double dt, foot_half_length, z_min, tilt_max;
    int32_t substeps, period, ds;
    long long B;
};

// the launch of srbdqp_fleet_advance_kernel on st (srbdqp_wrench_lat_ew.hip); map: the terrain instantiation over it (null: flat ground); landing_yaw [B]: the
// steered instantiation, heel and toe turned by it (null: along the world's x axis)
hipError_t launch_fleet_advance(const FleetArgs& a, hipStream_t st, const TerrainMap* map = nullptr, const double* landing_yaw = nullptr);

constexpr int kFleetTile = 64;   // robots per workgroup pass = its threads: one wave, one robot per lane
constexpr int kFleetRow = 13;    // LDS row of every staged array, in doubles: odd, so that a lane per row walks all banks

struct FleetBody {
    double mass, inertia[3], iinv[3], g;
    double foot[12], f[12];      // contact points (fixed in the world during the period) and the forces at them
    double push_t[3], push_a[3]; // the push: torque about the CoM, and force / mass
    double fsum_a[3];            // sum of the contact forces / mass
};

// d/dt of x = [rpy, com, omega (world), v, g] (tests/srbd_plant.py SrbdPlant.deriv): Euler-rate kinematics, I_w = R I_b R', R = Rz(yaw) Ry(pitch) Rx(roll)
__host__ __device__ __forceinline__ void fleet_deriv(const FleetBody& q, const double (&x)[13], double (&dx)[13]) {
    const double sr = sin(x[0]), cr = cos(x[0]), sp = sin(x[1]), cp = cos(x[1]), sy = sin(x[2]), cy = cos(x[2]);
    const double R[3][3] = {{cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr},
                            {sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr},
                            {-sp, cp * sr, cp * cr}};
    const double w[3] = {x[6], x[7], x[8]};
    double wb[3], hb[3], tau[3] = {q.push_t[0], q.push_t[1], q.push_t[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) wb[i] = R[0][i] * w[0] + R[1][i] * w[1] + R[2][i] * w[2];   // body rates R' omega
    // Euler rates E(rpy) R' omega
    const double tp = sp / cp;
    dx[0] = wb[0] + sr * tp * wb[1] + cr * tp * wb[2];
    dx[1] = cr * wb[1] - sr * wb[2];
    dx[2] = (sr * wb[1] + cr * wb[2]) / cp;
    dx[3] = x[9]; dx[4] = x[10]; dx[5] = x[11];
    // torque of the contact forces about the CoM where it is NOW: the points stay, the CoM moves
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double rx = q.foot[3 * c] - x[3], ry = q.foot[3 * c + 1] - x[4], rz = q.foot[3 * c + 2] - x[5];
        const double fx = q.f[3 * c], fy = q.f[3 * c + 1], fz = q.f[3 * c + 2];
        tau[0] += ry * fz - rz * fy;
        tau[1] += rz * fx - rx * fz;
        tau[2] += rx * fy - ry * fx;
    }
    // omega' = I_w^-1 (tau - omega x I_w omega), I_w omega = R (I_b wb), I_w^-1 = R I_b^-1 R'
#pragma unroll
    for (int i = 0; i < 3; ++i) hb[i] = q.inertia[i] * wb[i];
    double hw[3], n[3], nb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) hw[i] = R[i][0] * hb[0] + R[i][1] * hb[1] + R[i][2] * hb[2];
    n[0] = tau[0] - (w[1] * hw[2] - w[2] * hw[1]);
    n[1] = tau[1] - (w[2] * hw[0] - w[0] * hw[2]);
    n[2] = tau[2] - (w[0] * hw[1] - w[1] * hw[0]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nb[i] = q.iinv[i] * (R[0][i] * n[0] + R[1][i] * n[1] + R[2][i] * n[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) dx[6 + i] = R[i][0] * nb[0] + R[i][1] * nb[1] + R[i][2] * nb[2];
    dx[9] = q.fsum_a[0] + q.push_a[0];
    dx[10] = q.fsum_a[1] + q.push_a[1];
    dx[11] = q.fsum_a[2] + q.push_a[2] + x[12];
    dx[12] = 0.0;
}

// `substeps` classical Runge-Kutta steps of h under fleet_deriv (tests/srbd_plant.py SrbdPlant.step); x[12], gravity, stays
__host__ __device__ __forceinline__ void fleet_plant(const FleetBody& q, double (&x)[13], double h, int substeps) {
    for (int s = 0; s < substeps; ++s) {
        double k1[13], k2[13], k3[13], k4[13], y[13];
        fleet_deriv(q, x, k1);
#pragma unroll
        for (int k = 0; k < 13; ++k) y[k] = x[k] + 0.5 * h * k1[k];
        fleet_deriv(q, y, k2);
#pragma unroll
        for (int k = 0; k < 13; ++k) y[k] = x[k] + 0.5 * h * k2[k];
        fleet_deriv(q, y, k3);
#pragma unroll
        for (int k = 0; k < 13; ++k) y[k] = x[k] + h * k3[k];
        fleet_deriv(q, y, k4);
#pragma unroll
        for (int k = 0; k < 12; ++k) x[k] = x[k] + h / 6.0 * (k1[k] + 2.0 * k2[k] + 2.0 * k3[k] + k4[k]);
    }
}

// A workgroup (one wave) takes tiles of 64 consecutive robots.  Their inputs -- 13 + 12 + 12 + 3 (+ 6) doubles each -- are staged in LDS with coalesced loads
// (the forces are rows of 12 doubles inside the solve's [B][N][12]: 96 contiguous bytes each); lane r then holds robot r's 13 states in registers through the
// substeps' RK4, writes its new state and footholds back to its LDS rows, and the tile leaves with coalesced stores: in place, and into the roll-out's logs.
// A robot that is skipped keeps its rows, in memory (nothing of it is stored) and in the logs (which record what it holds).
//
// fleet_height: the height of the point (x, y, z) over the ground under it, what "fallen" compares with z_min; fleet_ground: the ground's height at (x, y), where a
// foot lands -- without a map z itself and the landing point's own z (`flat`).  ext: the kernel's extras, of which a TerrainMap is the map and a FleetSteer
// (below) is passed over
struct FleetSteer { const double* landing_yaw; };   // [B]: psi_L of srbdqp_mpc_inputs_steered_*, the heading a foot lands with

__device__ __forceinline__ double fleet_height(double, double, double z) { return z; }
template <class... REST>
__device__ __forceinline__ double fleet_height(double x, double y, double z, const TerrainMap& m, const REST&...) { double zg, n[3]; terrain_sample(m, x, y, zg, n); return z - zg; }
template <class... REST>
__device__ __forceinline__ double fleet_height(double x, double y, double z, const FleetSteer&, const REST&... rest) { return fleet_height(x, y, z, rest...); }
__device__ __forceinline__ double fleet_ground(double, double, double flat) { return flat; }
template <class... REST>
__device__ __forceinline__ double fleet_ground(double x, double y, double, const TerrainMap& m, const REST&...) { double zg, n[3]; terrain_sample(m, x, y, zg, n); return zg; }
template <class... REST>
__device__ __forceinline__ double fleet_ground(double x, double y, double flat, const FleetSteer&, const REST&... rest) { return fleet_ground(x, y, flat, rest...); }
// the heading of the touchdown among the extras, or null: feet along the world's x axis
__device__ __forceinline__ const double* fleet_landing_yaw() { return nullptr; }
template <class... REST>
__device__ __forceinline__ const double* fleet_landing_yaw(const FleetSteer& s, const REST&...) { return s.landing_yaw; }
template <class... REST>
__device__ __forceinline__ const double* fleet_landing_yaw(const TerrainMap&, const REST&... rest) { return fleet_landing_yaw(rest...); }

// MAP: nothing -- flat ground, the kernel of DESIGN.md section 17, whose text this parameter leaves what it was -- or one TerrainMap, the terrain instantiation
// (section 18): the ground is the map instead of the plane z = 0.  Two places differ: a foot that touches down stands at S(own xy).z, heel and toe each, and both
// "fallen" tests compare the CoM's height OVER the ground under it, x[5] - S(com xy).z, with z_min.  A FleetSteer behind it (or alone): the steered instantiations
// (section 20), in which heel and toe lie along the heading landing_yaw[b] -- steer_touchdown -- where the others lay them along the world's x axis.
template <int TILE, class... MAP>
__global__ __launch_bounds__(TILE) void srbdqp_fleet_advance_kernel(FleetArgs a, MAP... map) {
    static_assert(sizeof...(MAP) <= 2, "at most one map and one FleetSteer");
    constexpr bool STEER = (std::is_same<MAP, FleetSteer>::value || ...);
    constexpr int RW = kFleetRow;
    __shared__ double sx[TILE * RW], sft[TILE * RW], su[TILE * RW], slp[TILE * 3], spu[TILE * 6];
    __shared__ uint8_t swx[TILE], swf[TILE];      // robot r's state / footholds changed: store them
    const int t = threadIdx.x;
    const long long tiles = (a.B + TILE - 1) / TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long b0 = tile * TILE;
        const int nr = (int)((a.B - b0 < TILE) ? (a.B - b0) : TILE);
        for (int e = t; e < nr * 13; e += TILE) { const int r = e / 13, c = e - 13 * r; sx[RW * r + c] = a.x[b0 * 13 + e]; }
        for (int e = t; e < nr * 12; e += TILE) {
            const int r = e / 12, c = e - 12 * r;
            sft[RW * r + c] = a.feet[b0 * 12 + e];
            su[RW * r + c] = a.u0[(b0 + r) * a.u0_stride + c];
        }
        for (int e = t; e < nr * 3; e += TILE) slp[e] = a.landing[b0 * 3 + e];
        if (a.push) for (int e = t; e < nr * 6; e += TILE) spu[e] = a.push[b0 * 6 + e];
        __syncthreads();
        if (t < nr) {
            const long long b = b0 + t;
            double x[13];
            bool finite = true;
#pragma unroll
            for (int k = 0; k < 13; ++k) { x[k] = sx[RW * t + k]; finite = finite && isfinite(x[k]); }
            // 1. skip: a robot that fell, or whose state is not finite, holds; only its clock runs
            const bool run = finite && !(a.alive && a.alive[b] == 0);
            const double stamp0 = a.stamp[b];
            double stamp1;
            {
#pragma clang fp contract(off)   // one rounded addition, compared bit for bit
                stamp1 = stamp0 + a.dt;
            }
            a.stamp[b] = stamp1;                                             // 3. (stamps: 512 contiguous bytes per wave)
            bool wx = false, wf = false, up = run;
            if (run) {
                // (5.) a robot handed over outside the envelope has fallen already: it gets this period, and holds behind it whatever the period did
                const bool inside0 = !(fleet_height(x[3], x[4], x[5], map...) < a.z_min) && !(fabs(x[0]) > a.tilt_max) && !(fabs(x[1]) > a.tilt_max);
                // 2. plant: substeps of RK4 under the forces at the contact points
                FleetBody q;
                q.mass = a.mass; q.inertia[0] = a.inertia[0]; q.inertia[1] = a.inertia[1]; q.inertia[2] = a.inertia[2];
                if (a.robots) { const double* rec = a.robots + 8 * b; q.mass = rec[0]; q.inertia[0] = rec[1]; q.inertia[1] = rec[2]; q.inertia[2] = rec[3]; }
#pragma unroll
                for (int i = 0; i < 3; ++i) q.iinv[i] = 1.0 / q.inertia[i];
#pragma unroll
                for (int k = 0; k < 12; ++k) { q.foot[k] = sft[RW * t + k]; q.f[k] = su[RW * t + k]; }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    q.fsum_a[i] = (((q.f[i] + q.f[3 + i]) + q.f[6 + i]) + q.f[9 + i]) / q.mass;
                    q.push_t[i] = a.push ? spu[6 * t + i] : 0.0;
                    q.push_a[i] = a.push ? spu[6 * t + 3 + i] / q.mass : 0.0;
                }
                const double h = a.dt / (double)a.substeps;
                fleet_plant(q, x, h, a.substeps);
                wx = true;
#pragma unroll
                for (int k = 0; k < 13; ++k) sx[RW * t + k] = x[k];
                // 4. touchdown: a foot in the air at the step of stamp and down at the step of stamp' lands around the landing point, on the ground plane
                const bool stand = a.standing && a.standing[b];
                bool l0, r0, l1, r1;
                gait_flags(stand ? -1 : gait_phase0(stamp0, a.dt, a.period), 0, a.period, a.ds, l0, r0);
                gait_flags(stand ? -1 : gait_phase0(stamp1, a.dt, a.period), 0, a.period, a.ds, l1, r1);
                const bool left = !l0 && l1, right = !r0 && r1;
                if (left || right) {
                    const int c0 = left ? 0 : 6;                                   // contacts 0, 1 (left heel, toe) or 2, 3
                    const double lx = slp[3 * t], ly = slp[3 * t + 1], lz = slp[3 * t + 2];
                    if constexpr (STEER) {
                        double heel[2], toe[2];
                        steer_touchdown(lx, ly, a.foot_half_length, fleet_landing_yaw(map...)[b], heel, toe);
                        sft[RW * t + c0] = heel[0]; sft[RW * t + c0 + 1] = heel[1]; sft[RW * t + c0 + 2] = fleet_ground(heel[0], heel[1], lz, map...);
                        sft[RW * t + c0 + 3] = toe[0]; sft[RW * t + c0 + 4] = toe[1]; sft[RW * t + c0 + 5] = fleet_ground(toe[0], toe[1], lz, map...);
                    } else {
                        sft[RW * t + c0] = lx - a.foot_half_length; sft[RW * t + c0 + 1] = ly; sft[RW * t + c0 + 2] = fleet_ground(lx - a.foot_half_length, ly, lz, map...);
                        sft[RW * t + c0 + 3] = lx + a.foot_half_length; sft[RW * t + c0 + 4] = ly; sft[RW * t + c0 + 5] = fleet_ground(lx + a.foot_half_length, ly, lz, map...);
                    }
                    wf = true;
                }
                // 5. fallen: it holds from the next period on
                bool ok = true;
#pragma unroll
                for (int k = 0; k < 12; ++k) ok = ok && isfinite(x[k]);
                up = inside0 && ok && !(fleet_height(x[3], x[4], x[5], map...) < a.z_min) && !(fabs(x[0]) > a.tilt_max) && !(fabs(x[1]) > a.tilt_max);
            }
            swx[t] = wx; swf[t] = wf;
            if (a.alive && !up) a.alive[b] = 0;
            if (a.status_log) a.status_log[b] = a.status[b];
            if (a.iters_log) a.iters_log[b] = a.iters[b];
        }
        __syncthreads();
        for (int e = t; e < nr * 13; e += TILE) {
            const int r = e / 13, c = e - 13 * r;
            const double v = sx[RW * r + c];
            if (swx[r]) a.x[b0 * 13 + e] = v;
            if (a.x_log) a.x_log[b0 * 13 + e] = v;
        }
        for (int e = t; e < nr * 12; e += TILE) {
            const int r = e / 12, c = e - 12 * r;
            const double v = sft[RW * r + c];
            if (swf[r]) a.feet[b0 * 12 + e] = v;
            if (a.feet_log) a.feet_log[b0 * 12 + e] = v;
            if (a.u0_log) a.u0_log[b0 * 12 + e] = su[RW * r + c];
        }
        __syncthreads();
    }
}

}  // namespace srbdqp
