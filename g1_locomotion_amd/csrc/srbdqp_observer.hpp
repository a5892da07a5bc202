// The momentum observer of a fleet (include/srbdqp_cascade.h, srbdqp_wrench_observer_*): from the state before and behind one control
// period, the contact points and the first-step forces the period ran under, the wrench on the body that the forces do not explain -- a push, a payload --,
// filtered, clamped and laid out along the horizon as the external wrench of the next solve (srbdqp_set_external_wrench's layout, section 16).
//
// observer_measure and observer_update are __host__ __device__, like fleet_deriv, and need nothing of HIP: a host compiler builds them from this header alone
// (tests/test_observer_cpu.py does, against tests/observer_twin.py).  The kernel below them is a template so that it is emitted only where it is instantiated:
// in srbdqp_wrench_lat_ew.hip, the library's second code object, as the fleet's and the terrain's kernels are; srbdqp.hip sees ObserverArgs and the launcher.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SRBDQP_OBS_HD __host__ __device__ __forceinline__
#else
#define SRBDQP_OBS_HD inline
#endif

namespace srbdqp {

// L(x) = R(rpy) diag(I_b) R(rpy)' omega: the angular momentum about the CoM in the world frame, R = Rz(yaw) Ry(pitch) Rx(roll) as in fleet_deriv
SRBDQP_OBS_HD void observer_momentum(const double (&inertia)[3], const double (&x)[13], double (&L)[3]) {
    const double sr = sin(x[0]), cr = cos(x[0]), sp = sin(x[1]), cp = cos(x[1]), sy = sin(x[2]), cy = cos(x[2]);
    const double R[3][3] = {{cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr},
                            {sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr},
                            {-sp, cp * sr, cp * cr}};
    double hb[3];
    for (int i = 0; i < 3; ++i) hb[i] = inertia[i] * (R[0][i] * x[6] + R[1][i] * x[7] + R[2][i] * x[8]);   // I_b (R' omega)
    for (int i = 0; i < 3; ++i) L[i] = R[i][0] * hb[0] + R[i][1] * hb[1] + R[i][2] * hb[2];
}

// w = [tau_meas, f_meas]: the wrench on the body over one period of dt that the contact forces f at the points p do not explain (world frame, torque about
// the CoM first).  x0: the state before the period (x0[12]: gravity), x1: behind it; p: the contact points the forces acted at.
//   f_meas   = m (v1 - v0) / dt - sum f_i - m g e_z
//   cbar     = c0 + dt (2 v0 + v1) / 6                 the mean CoM of a period of constant acceleration
//   tau_meas = (L(x1) - L(x0)) / dt - sum (p_i - cbar) x f_i
SRBDQP_OBS_HD void observer_measure(double mass, const double (&inertia)[3], double dt, const double (&x0)[13], const double (&x1)[13], const double (&p)[12],
                                    const double (&f)[12], double (&w)[6]) {
    double L0[3], L1[3], cb[3], tc[3] = {0.0, 0.0, 0.0};
    observer_momentum(inertia, x0, L0);
    observer_momentum(inertia, x1, L1);
    for (int i = 0; i < 3; ++i) {
        const double fs = ((f[i] + f[3 + i]) + f[6 + i]) + f[9 + i];
        w[3 + i] = mass * (x1[9 + i] - x0[9 + i]) / dt - fs;
        cb[i] = x0[3 + i] + dt * (2.0 * x0[9 + i] + x1[9 + i]) / 6.0;
    }
    w[5] = w[5] - mass * x0[12];
    for (int c = 0; c < 4; ++c) {
        const double rx = p[3 * c] - cb[0], ry = p[3 * c + 1] - cb[1], rz = p[3 * c + 2] - cb[2];
        const double fx = f[3 * c], fy = f[3 * c + 1], fz = f[3 * c + 2];
        tc[0] += ry * fz - rz * fy;
        tc[1] += rz * fx - rx * fz;
        tc[2] += rx * fy - ry * fx;
    }
    for (int i = 0; i < 3; ++i) w[i] = (L1[i] - L0[i]) / dt - tc[i];
}

// the filter: w_est += gain (w_meas - w_est), then the torques clamped to +-torque_max, then the forces to +-force_max (fmin / fmax: a value that is not a
// number leaves at a bound, so that what the next solve reads always passes the rule of srbdqp_set_external_wrench)
SRBDQP_OBS_HD void observer_update(double gain, double torque_max, double force_max, const double (&w_meas)[6], double (&w_est)[6]) {
    for (int i = 0; i < 6; ++i) {
        const double v = w_est[i] + gain * (w_meas[i] - w_est[i]);
        const double m = i < 3 ? torque_max : force_max;
        w_est[i] = fmin(fmax(v, -m), m);
    }
}

struct ObserverArgs {
    const double* x_prev;    // [B][13]  the state before the period
    const double* x_next;    // [B][13]  ... behind it
    const double* feet;      // [B][12]  the contact points the forces acted at
    const double* u0;        // the forces: robot b's twelve at u0 + b * u0_stride
    long long u0_stride;
    const uint8_t* alive;    // [B] or null, as it stands behind the period
    const double* robots;    // per-robot records (srbdqp_robot, 8 doubles) in place of mass / inertia, or null
    double* w_est;           // [B][6]   in/out
    double* ew;              // [B][N][6] or null: w_est' decay^k
    double* w_log;           // [B][6] or null: the roll-out's record of w_est'
    double mass, inertia[3];
    double dt, gain, decay, torque_max, force_max;
    int32_t N;
    int32_t fill_only;       // non-zero: no measurement, every robot keeps its w_est (x_prev ... u0 are not read); ew is written from it
    long long B;
};

// the launch of srbdqp_wrench_observer_kernel on st (srbdqp_wrench_lat_ew.hip)
#if defined(__HIPCC__)
hipError_t launch_wrench_observer(const ObserverArgs& a, hipStream_t st);

constexpr int kObserverTile = 64;   // robots per workgroup pass = its threads: one wave, one robot per lane (srbdqp_fleet_advance_kernel's tiles)
constexpr int kObserverRow = 13;    // LDS row of every staged input, in doubles: odd, so that a lane per row walks all banks
constexpr int kObserverWRow = 7;    // ... and of the estimate's six

// A workgroup (one wave) takes tiles of 64 consecutive robots.  The two states, the contact points, the forces and the estimate are staged in LDS with
// coalesced loads; lane r measures and filters robot r and writes its estimate back to its LDS row; the tile's estimates and its 64 N 6 doubles of ew, which
// are contiguous, leave with coalesced stores -- entry (r, k, c) is w_est'[r][c] times decay k times over, one rounded product after the other.
template <int TILE>
__global__ __launch_bounds__(TILE) void srbdqp_wrench_observer_kernel(ObserverArgs a) {
    constexpr int RW = kObserverRow, WW = kObserverWRow;
    __shared__ double sx0[TILE * RW], sx1[TILE * RW], sft[TILE * RW], su[TILE * RW], sw[TILE * WW];
    const int t = threadIdx.x;
    const long long tiles = (a.B + TILE - 1) / TILE;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long b0 = tile * TILE;
        const int nr = (int)((a.B - b0 < TILE) ? (a.B - b0) : TILE);
        // every load of the tile is in flight before the first LDS store (a lane's share: at most 13 + 13 + 12 + 12 + 6 doubles, in registers): one wave has
        // nothing else to hide a round trip to memory behind, and a loop that stored each element as it came would pay 31 of them in a row
        double vx0[13], vx1[13], vf[12], vu[12], vw[6];
        if (!a.fill_only) {
#pragma unroll
            for (int i = 0; i < 13; ++i) { const int e = t + TILE * i; if (e < nr * 13) { vx0[i] = a.x_prev[b0 * 13 + e]; vx1[i] = a.x_next[b0 * 13 + e]; } }
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const int e = t + TILE * i, r = e / 12, c = e - 12 * r;
                if (e < nr * 12) { vf[i] = a.feet[b0 * 12 + e]; vu[i] = a.u0[(b0 + r) * a.u0_stride + c]; }
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) { const int e = t + TILE * i; if (e < nr * 6) vw[i] = a.w_est[b0 * 6 + e]; }
        if (!a.fill_only) {
#pragma unroll
            for (int i = 0; i < 13; ++i) { const int e = t + TILE * i, r = e / 13, c = e - 13 * r; if (e < nr * 13) { sx0[RW * r + c] = vx0[i]; sx1[RW * r + c] = vx1[i]; } }
#pragma unroll
            for (int i = 0; i < 12; ++i) { const int e = t + TILE * i, r = e / 12, c = e - 12 * r; if (e < nr * 12) { sft[RW * r + c] = vf[i]; su[RW * r + c] = vu[i]; } }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) { const int e = t + TILE * i, r = e / 6, c = e - 6 * r; if (e < nr * 6) sw[WW * r + c] = vw[i]; }
        __syncthreads();
        if (t < nr && !a.fill_only) {
            const long long b = b0 + t;
            double x0[13], x1[13];
            bool finite = true;
#pragma unroll
            for (int k = 0; k < 13; ++k) { x0[k] = sx0[RW * t + k]; x1[k] = sx1[RW * t + k]; finite = finite && isfinite(x0[k]) && isfinite(x1[k]); }
            // a robot that is down, or whose state is not finite, keeps its estimate
            if (finite && !(a.alive && a.alive[b] == 0)) {
                double mass = a.mass, inertia[3] = {a.inertia[0], a.inertia[1], a.inertia[2]};
                if (a.robots) { const double* rec = a.robots + 8 * b; mass = rec[0]; inertia[0] = rec[1]; inertia[1] = rec[2]; inertia[2] = rec[3]; }
                double p[12], f[12], wm[6], we[6];
#pragma unroll
                for (int k = 0; k < 12; ++k) { p[k] = sft[RW * t + k]; f[k] = su[RW * t + k]; }
#pragma unroll
                for (int k = 0; k < 6; ++k) we[k] = sw[WW * t + k];
                observer_measure(mass, inertia, a.dt, x0, x1, p, f, wm);
                observer_update(a.gain, a.torque_max, a.force_max, wm, we);
#pragma unroll
                for (int k = 0; k < 6; ++k) sw[WW * t + k] = we[k];
            }
        }
        __syncthreads();
        for (int e = t; e < nr * 6; e += TILE) {
            const int r = e / 6, c = e - 6 * r;
            const double v = sw[WW * r + c];
            if (!a.fill_only) a.w_est[b0 * 6 + e] = v;
            if (a.w_log) a.w_log[b0 * 6 + e] = v;
        }
        if (a.ew) {
            // a lane keeps its place (k, c) in a robot's row of 6 N doubles and walks the tile's robots: 64 consecutive doubles per store, row after row
            const int row = 6 * a.N;
            double* const out = a.ew + b0 * row;
            for (int q = t; q < row; q += TILE) {
                const int k = q / 6, c = q - 6 * k;
#pragma unroll 4
                for (int r = 0; r < nr; ++r) {
                    double s = sw[WW * r + c];
                    for (int j = 0; j < k; ++j) s = s * a.decay;
                    out[r * row + q] = s;
                }
            }
        }
        __syncthreads();
    }
}
#endif  // __HIPCC__

}  // namespace srbdqp
