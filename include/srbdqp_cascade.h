/* srbdqp_cascade.h -- the steps either side of the QP in the reference's control cascade, batched on the GPU
 * (SURVEY.md 8(f) rows 2, 3 and 4).  Same library (libsrbdqp.so), same handle, same error convention as srbdqp.h.
 *
 *   srbdqp_swing_*            replaces  SwingTrajectory.calculate_coeff / calculate_position_xy / calculate_position_z /
 *                             calculate_velocity_z / calculate_acceleration_z
 *                             (g1_mujoco_sim/src/swing_trajectory.py:38-89; called from ros_run_simulation.py:246-256,
 *                             300-312), for B feet at once.
 *   srbdqp_wbid_reference_*   replaces the arithmetic of WBID.setReference(t, x_opt1, u_opt0, foot_positions_curr)
 *                             (g1_mujoco_sim/src/wbid.py:232-297): everything it computes before handing the
 *                             references to the OpenSoT tasks, for B robots at once.
 *
 * Host-buffer variants copy in and out and return when the outputs are valid; *_device_* variants take device pointers
 * and a hipStream_t (NULL = the handle's stream) and return after the launch.
 */
#ifndef SRBDQP_CASCADE_H
#define SRBDQP_CASCADE_H

#include "srbdqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* swing_trajectory.py:50 (downward landing velocity) and :58 (share of the x-y distance covered in the first half) */
#define SRBDQP_SWING_FINAL_VELOCITY_Z (-0.02)
#define SRBDQP_SWING_FIRST_HALF_SHARE 0.80

/* p_start, p_final [B][3]; z_middle, progress [B]; pos [B][3]; vel_z, acc_z [B] (optional); coeff [B][7] (optional:
 * the polynomial's coefficients, lowest power first, = SwingTrajectory.coeff). */
int srbdqp_swing_f64(srbdqp_handle* h, int64_t B, const double* p_start, const double* p_final, const double* z_middle,
                     const double* progress, double final_velocity_z, double first_half_share, double* pos,
                     double* vel_z, double* acc_z, double* coeff);
int srbdqp_swing_device_f64(srbdqp_handle* h, int64_t B, const double* p_start, const double* p_final,
                            const double* z_middle, const double* progress, double final_velocity_z,
                            double first_half_share, double* pos, double* vel_z, double* acc_z, double* coeff,
                            void* stream);

/* x_next [B][13] (= x_opt1[1]); u0 [B][12] (= u_opt0); foot [B][12] (current contact points, srbdqp.h order);
 * R [B][9] row-major base orientation (tf euler_matrix 'sxyz'); base_vel [B][6] = [v, omega];
 * base_acc [B][6] = [0, I^-1 sum_i r_i x omega]; com_acc [B][3] = sum of forces / mass + gravity.
 * as_written != 0 sums the forces the way wbid.py:290 does (np.reshape(u_opt0, (3, 4)) summed along axis 1: groups of
 * four consecutive entries, not the per-axis sums); 0 gives the per-axis sums.  Mass, inertia: the handle's config;
 * gravity: x_next[12] is NOT used, the constant -9.80665 of wbid.py:286 is. */
int srbdqp_wbid_reference_f64(srbdqp_handle* h, int64_t B, const double* x_next, const double* u0, const double* foot,
                              int32_t as_written, double* R, double* base_vel, double* base_acc, double* com_acc);
int srbdqp_wbid_reference_device_f64(srbdqp_handle* h, int64_t B, const double* x_next, const double* u0,
                                     const double* foot, int32_t as_written, double* R, double* base_vel,
                                     double* base_acc, double* com_acc, void* stream);

/* ---- the step BEFORE the QP: gait schedule + landing position + the QP's input horizons, for B
 * robots at once.  What the reference's MPC node does between receiving /srbd_current and calling MPC.update()
 * (ros_run_simulation.py:214-218, 378-399 consume its outputs: contacts[i].active and landing_position; run_simulation.py:
 * 73-101 builds the same horizons for one robot).  The schedule itself is inside the absent module: this is the builder's own
 * design (fixed-period alternating single support with a double-support overlap, Raibert-style landing point), the same
 * one g1_locomotion_amd/msgs.py (AlternatingGait, MpcNode.step) runs on the host for one robot.
 *
 * Outputs are laid out exactly as srbdqp_solve_batch_device_f64 takes them, so a fleet's control step stays on the device:
 *   srbdqp_mpc_inputs_device_f64 -> srbdqp_solve_batch_device_f64(..., pcom) -> srbdqp_wbid_reference_device_f64. */
typedef struct srbdqp_gait {
    int32_t struct_size;          /* = sizeof(srbdqp_gait) */
    int32_t period_steps;         /* horizon steps one foot swings (0.25 s / dt, ros_run_simulation.py:148) */
    int32_t double_support_steps; /* steps of double support at the start of every half period */
    int32_t reserved0;
    double com_target[3];         /* CoM reference when v_ref = 0 (run_simulation.py:81) */
    double hip_offset_y;          /* lateral offset of the landing point from the CoM */
} srbdqp_gait;

/* x0 [B][13] measured state; feet [B][12] current contact-point positions (srbdqp.h order); stamp [B] seconds;
 * v_ref [B][2] commanded planar velocity; standing [B] non-zero = all four contacts in stance (may be NULL = walking).
 * Horizon N and dt: the handle's config.  Outputs: x_ref [B][N][13], foot [B][N][12], contact [B][N][4], pcom [B][N][3],
 * landing [B][3] (may be NULL): landing position of the foot that swings (or swings next) at the first step. */
int srbdqp_mpc_inputs_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp,
                          const double* v_ref, const uint8_t* standing, const srbdqp_gait* gait,
                          double* x_ref, double* foot, uint8_t* contact, double* pcom, double* landing);
int srbdqp_mpc_inputs_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp,
                                 const double* v_ref, const uint8_t* standing, const srbdqp_gait* gait,
                                 double* x_ref, double* foot, uint8_t* contact, double* pcom, double* landing, void* stream);

/* ---- from control step t to step t + 1: a fleet's roll-out on the device.
 *
 * srbdqp_fleet_advance_* is one control period of B robots between two solves, in this order:
 *   1. skip       a robot with alive == 0, or with a non-finite entry in x, gets alive = 0 and nothing else written (its stamp still advances);
 *   2. plant      `substeps` RK4 steps of h = dt / substeps of the nonlinear single rigid body: Euler-rate kinematics, I_w = R I_b R' with
 *                 R = Rz(yaw) Ry(pitch) Rx(roll), the gyroscopic term omega x I_w omega, the forces u0 at the contact points `feet` held fixed in the
 *                 world, v' = sum f / m + f_push / m + g e_z with g = x[12], the push's torque added to sum r x f;
 *   3. stamp      stamp' = stamp + dt (one rounded addition);
 *   4. touchdown  the left foot (contacts 0, 1) or the right foot (contacts 2, 3) whose first-step flag under the gait is 0 at stamp and 1 at stamp'
 *                 moves: heel = landing - (foot_half_length, 0, 0), toe = landing + (foot_half_length, 0, 0), z as in landing (the ground plane).
 *                 The gait is the schedule of srbdqp_mpc_inputs_*: step index floor(stamp / dt + 1e-9), gait.period_steps,
 *                 gait.double_support_steps, standing.  Every other foot stays;
 *   5. fallen     a new CoM height below z_min, |roll| or |pitch| above tilt_max, or a non-finite state: alive = 0.  The state of this period is still
 *                 written; the robot holds from the next period on.  A robot handed over with such a height or tilt has fallen already: it gets
 *                 this period like any other and alive = 0 behind it, wherever the period took it.
 * dt, and mass and inertia where the handle has no robot records (srbdqp_set_robots: robot b's own, as srbdqp_wbid_reference_* reads them): the handle's
 * config.  The MPC does not know the push (srbdqp_fleet_rollout_observed_* below estimates it from what the plant did). */
typedef struct srbdqp_fleet_settings {
    int32_t struct_size;          /* = sizeof(srbdqp_fleet_settings) */
    int32_t substeps;             /* RK4 steps per control period (10) */
    double foot_half_length;      /* heel and toe lie this far behind and ahead of the landing point (0.085: synth.py's spacing) */
    double z_min;                 /* fallen: CoM height below it (0.3) */
    double tilt_max;              /* fallen: |roll| or |pitch| above it, rad (1.0: keeps the Euler angles away from their singularity) */
    srbdqp_gait gait;             /* the schedule, as srbdqp_mpc_inputs_* takes it */
} srbdqp_fleet_settings;

/* The defaults above into *s; s->struct_size says how large the caller's struct is (checked before anything is written).  gait: period_steps 6,
 * double_support_steps 1, hip_offset_y 0.0645, com_target (0, 0, 0) -- the caller's to fill. */
int srbdqp_fleet_default_settings(srbdqp_fleet_settings* s);

/* x [B][13], feet [B][12], stamp [B]: in/out.  u0: the first-step forces, robot b's twelve doubles at u0 + b * u0_stride (u0_stride >= 12, in doubles:
 * 12 N reads u_out[b][0] of a solve in place).  landing [B][3] as srbdqp_mpc_inputs_* wrote it.  standing [B], push [B][6] (world wrench on the body during
 * this period, torque about the CoM first as in srbdqp_set_external_wrench), alive [B] (in/out): each may be NULL. */
int srbdqp_fleet_advance_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                             const double* landing, const uint8_t* standing, const double* push, uint8_t* alive,
                             const srbdqp_fleet_settings* cfg);
int srbdqp_fleet_advance_device_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                                    const double* landing, const uint8_t* standing, const double* push, uint8_t* alive,
                                    const srbdqp_fleet_settings* cfg, void* stream);

/* ---- the ground under the fleet: a height map on the handle, which the roll-out walks on.
 *
 * heights_host [ny][nx] doubles, x fastest: node (i, j) lies at (x0 + i cell, y0 + j cell).  The library checks and copies the map; NULL (t or heights_host)
 * clears it.  Replacing or clearing a map first waits for every stream of the handle.  srbdqp_destroy frees it.  Refused (SRBDQP_E_INVALID, nothing copied, the
 * map that was set stays): a wrong struct_size; nx or ny below 2, nx ny above 2^24; a cell that is not finite and positive; an origin that is not finite; a
 * height that is not finite; two neighbouring heights, along x or along y, that differ by more than 1.2 cell -- which keeps gx^2 + gy^2 <= 2.88 below, so that
 * every normal the map can produce has n_z >= 0.5, the rule of srbdqp_set_contact_normals, and the device may produce normals without a host check.
 *
 * A map changes srbdqp_fleet_advance_* and srbdqp_fleet_rollout_* (below) and makes the srbdqp_terrain_* calls available; every solve on the handle is untouched.
 *
 * The sample S(x, y) -> (z, n), every step one rounded fp64 operation (no fused multiply-add):
 *   u = (x - x0) / cell clamped to [0, nx - 1];  i = min(floor(u), nx - 2);  fx = u - i;      v, j, fy: the same along y
 *   h00 = h[j][i], h10 = h[j][i+1], h01 = h[j+1][i], h11 = h[j+1][i+1]
 *   a = h00 + fx (h10 - h00);  b = h01 + fx (h11 - h01);  z = a + fy (b - a)
 *   gx = ((h10 - h00) + fy ((h11 - h01) - (h10 - h00))) / cell;   gy = ((h01 - h00) + fx ((h11 - h10) - (h01 - h00))) / cell
 *   n = (-gx, -gy, 1) / sqrt((gx gx + gy gy) + 1)
 * A point off the map is the clamped point.  A coordinate that is not finite gives z = NaN and n = (0, 0, 1). */
typedef struct srbdqp_terrain {
    int32_t struct_size;          /* = sizeof(srbdqp_terrain) */
    int32_t nx, ny;               /* nodes along x and along y, >= 2 each */
    int32_t reserved0;
    double x0, y0;                /* node (0, 0) */
    double cell;                  /* node spacing, m */
} srbdqp_terrain;

int srbdqp_set_terrain(srbdqp_handle* h, const srbdqp_terrain* t, const double* heights_host);

/* S at M points: xy [M][2] -> z [M], normal [M][3] (may be NULL).  One point per lane.  Without a map: SRBDQP_E_INVALID. */
int srbdqp_terrain_sample_f64(srbdqp_handle* h, int64_t M, const double* xy, double* z, double* normal);
int srbdqp_terrain_sample_device_f64(srbdqp_handle* h, int64_t M, const double* xy, double* z, double* normal, void* stream);

/* Between srbdqp_mpc_inputs_* and the solve: feet [B][12] (as handed to srbdqp_mpc_inputs_*), x_ref [B][N][13] in/out, normals [B][N][12] out, in the layout
 * of srbdqp_set_contact_normals.  The normal of contact i of robot b is S(feet xy of i).n at every step (a swing contact's too: it keeps its old point until it
 * lands); x_ref[b][k][5] += (((z0 + z1) + z2) + z3) 0.25 over the z of `feet` as handed in: the height reference follows the ground the robot stands on.
 * N: the handle's horizon.  Without a map: SRBDQP_E_INVALID. */
int srbdqp_terrain_inputs_f64(srbdqp_handle* h, int64_t B, const double* feet, double* x_ref, double* normals);
int srbdqp_terrain_inputs_device_f64(srbdqp_handle* h, int64_t B, const double* feet, double* x_ref, double* normals, void* stream);

/* With a map set, srbdqp_fleet_advance_* differs in two places: at a touchdown the heel and the toe each get z = S(own xy).z where landing's z is copied on
 * flat ground, and both "fallen" tests compare x[5] - S(com xy).z, the height over the ground, with z_min.  And srbdqp_fleet_rollout_* enqueues per step
 *   srbdqp_mpc_inputs_device_f64 -> srbdqp_terrain_inputs_device_f64, into a normals buffer of the handle's roll-out allocation -> the fp64 batch solve on the
 *   general kernel with those normals as the normals of this call (every restart pass reads them; nothing is set on the handle) -> srbdqp_flush on a
 *   SRBDQP_FLAG_DEFER_TAIL handle -> the terrain plant step.
 * Such a roll-out is refused (SRBDQP_E_INVALID before any launch, in the words of the handle's state "while a terrain is set") beside robot records, weights,
 * an external wrench or handle-level normals, on a live horizon, with rank-aware steps, at N = 24 and with a srbdqp_config.kernel that bars the general kernel:
 * no instantiation reads normals beside those.  Not modelled: ground reaction or sliding in the plant (the forces are the QP's), footholds predicted along the
 * horizon (srbdqp_fleet_rollout_previewed_* below previews them), per-robot map offsets, feet turned with yaw (srbdqp_fleet_advance_steered_* below turns them), terrain under the swing trajectory, fp32, ragged fleets. */

/* T control steps of B robots: for t = 0 ... T - 1, srbdqp_mpc_inputs_device_f64 -> the solve, exactly the launches srbdqp_solve_batch_device_f64 makes
 * for this handle, with pcom from the inputs -> srbdqp_fleet_advance_device_f64, enqueued on `stream` without a host synchronisation (plain launches: no
 * graph, no persistent kernel).  On a SRBDQP_FLAG_DEFER_TAIL handle srbdqp_flush follows every solve: the plant needs complete forces.
 *   x [B][13], feet [B][12], stamp [B], alive [B] (may be NULL): in/out.  v_ref [B][2], standing [B] (may be NULL): constant over the call.
 *   push [T][B][6] or NULL.  Logs, each may be NULL: x_log [T+1][B][13] and feet_log [T+1][B][12] (entry 0: as passed in; t + 1: behind period t),
 *   u0_log [T][B][12] (the forces period t ran under), status_log, iters_log [T][B] (of the solve of step t).
 * Robot records and weights set on the handle are honoured (the solves read them; the plant reads mass and inertia).  A handle with an external wrench or
 * contact normals set is refused (SRBDQP_E_INVALID): the plant is flat ground and the MPC's wrench is not the plant's.  (With a map set, srbdqp_set_terrain
 * above, the fleet walks on it and the list of refusals is the one given there.)  The horizon buffers (x_ref, foot,
 * contact, pcom, landing, u, x_out, status, iters for B robots) belong to the handle: allocated at the first roll-out, grown when a larger B asks,
 * released by srbdqp_destroy.  Nothing is set or cleared on the handle.  B or T < 1, a bad struct_size, substeps < 1, a setting that is not finite or
 * not positive, an invalid gait: SRBDQP_E_INVALID before any launch. */
int srbdqp_fleet_rollout_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                                    const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                    double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log, void* stream);
/* ... through host buffers: returns with the results in place. */
int srbdqp_fleet_rollout_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                             const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                             double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log);

/* ---- a fleet that feels its pushes: the momentum observer and the roll-out whose solves read it.
 *
 * The measurement over one control period, from the state before it x0, the state behind it x1, the contact points p_i the forces acted at (the feet BEFORE
 * any touchdown), the held first-step forces f_i, mass m, body inertia I_b (robot b's record where srbdqp_set_robots is set, as in the plant step), the
 * handle's dt and g = x0[12]:
 *   f_meas   = m (v1 - v0) / dt - sum f_i - m g e_z
 *   cbar     = c0 + dt (2 v0 + v1) / 6           (the mean CoM of a period of constant acceleration)
 *   L(x)     = R(rpy) diag(I_b) R(rpy)' omega,   R = Rz Ry Rx as in the plant
 *   tau_meas = (L(x1) - L(x0)) / dt - sum (p_i - cbar) x f_i
 *   w_meas   = [tau_meas, f_meas]                (torque first, world frame, about the CoM: the layout of srbdqp_set_external_wrench)
 * Under the library's own plant the forces are held, so v' is constant: f_meas and cbar are exact and tau_meas is exact up to the RK4 error (1e-6 N m at 10
 * substeps); for a real robot it is the usual O(dt^2) momentum observer.
 * The filter, in this order: w_est' = w_est + gain (w_meas - w_est); the torque components clamped to +-torque_max; the force components to +-force_max.
 * The wrench of the next solve: ew[b][k] = w_est'_b decay^k, k = 0 ... N - 1, by repeated multiplication (s_0 = w_est', s_{k+1} = s_k decay).
 * A robot keeps its w_est (ew is still written, from the kept value) when alive == 0 as it stands behind the period, or x0 or x1 has a non-finite entry. */
typedef struct srbdqp_observer_settings {
    int32_t struct_size;          /* = sizeof(srbdqp_observer_settings) */
    int32_t reserved0;
    double gain;                  /* of the first-order filter, in (0, 1] (0.5) */
    double horizon_decay;         /* of the estimate along the horizon, in [0, 1] (1.0: the push is expected to last) */
    double torque_max;            /* clamp of the torque components, N m: finite, positive, at most SRBDQP_EXT_WRENCH_MAX (50) */
    double force_max;             /* clamp of the force components, N: the same rule (200) */
} srbdqp_observer_settings;

/* The defaults above into *s; s->struct_size says how large the caller's struct is (checked before anything is written). */
int srbdqp_observer_default_settings(srbdqp_observer_settings* s);

/* x_prev, x_next [B][13]; feet_prev [B][12]; u0: robot b's twelve doubles at u0 + b * u0_stride (u0_stride >= 12); alive [B] or NULL; w_est [B][6] in/out;
 * ew_out [B][N][6] or NULL (N: the handle's horizon; at B = 1 the array srbdqp_update_wrench_f64 takes).  A wrong struct_size, gain outside (0, 1], decay
 * outside [0, 1], a bound that is not finite, not positive or above SRBDQP_EXT_WRENCH_MAX: SRBDQP_E_INVALID before any launch -- so the kernel's own wrench
 * check never fires on an observer's output.  srbdqp_kernel_name: wrench_observer_f64. */
int srbdqp_wrench_observer_f64(srbdqp_handle* h, int64_t B, const double* x_prev, const double* x_next, const double* feet_prev, const double* u0,
                               int64_t u0_stride, const uint8_t* alive, const srbdqp_observer_settings* cfg, double* w_est, double* ew_out);
int srbdqp_wrench_observer_device_f64(srbdqp_handle* h, int64_t B, const double* x_prev, const double* x_next, const double* feet_prev, const double* u0,
                                      int64_t u0_stride, const uint8_t* alive, const srbdqp_observer_settings* cfg, double* w_est, double* ew_out,
                                      void* stream);

/* srbdqp_fleet_rollout_* on flat ground whose solves read the observer's estimate.  Per step: srbdqp_mpc_inputs_device_f64 -> the fp64 batch solve on the
 * general kernel with the handle's wrench buffer as the wrench of this call (wrench_f64_n<N>_ew, which reads the handle's weights and robot records too; every
 * restart pass, deferred ones on the tail stream included, reads the same buffer) -> srbdqp_flush on a SRBDQP_FLAG_DEFER_TAIL handle -> the flat plant step ->
 * the observer over the period that just ran, which writes the wrench of the next solve.  The solve of step t reads decay^k w_est as it stands before period
 * t (at t = 0 the caller's): the estimate of period t serves solve t + 1.
 *   obs: the observer's settings.  w_est [B][6] in/out, required.  w_log [T][B][6] or NULL: the estimate behind period t.  Everything else as in
 *   srbdqp_fleet_rollout_*; chunks compose bit for bit with w_est carried by the caller.
 * Refused (SRBDQP_E_INVALID before any launch): what srbdqp_fleet_rollout_* refuses; bad settings; w_est NULL; contact normals or a handle-level wrench set, a
 * live horizon, rank-aware steps, N = 24, a srbdqp_config.kernel that bars the general kernel ("... in an observed roll-out"); a terrain set on the handle (no
 * instantiation reads normals beside a wrench).  Robot records and weights are honoured.  The wrench buffer and a two-slot ring of states and footholds
 * (used where the caller passes no x_log / feet_log) join the handle's roll-out allocation at the first observed roll-out.
 * Not modelled: terrain, fp32, ragged fleets, the swing leg's inertia, a prediction of the push beyond the geometric decay. */
int srbdqp_fleet_rollout_observed_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                                             const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                             double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                             const srbdqp_observer_settings* obs, double* w_est, double* w_log, void* stream);
int srbdqp_fleet_rollout_observed_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* v_ref,
                                      const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                      double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                      const srbdqp_observer_settings* obs, double* w_est, double* w_log);

/* ---- a fleet that steers: yaw-rate commands and turned footholds.
 *
 * srbdqp_mpc_inputs_steered_* is srbdqp_mpc_inputs_* under command [B][3] = (vx, vy, wz) -- planar velocity in the robot's HEADING frame, m/s, and yaw rate,
 * rad/s -- in place of v_ref, with one more output, landing_yaw [B] (may be NULL).  x_ref, foot, contact, pcom, landing: the layout of srbdqp_mpc_inputs_*.
 * With psi0 = x0[2], Rz(th) the planar rotation, v_w(th) = Rz(th) (vx, vy) = (cos th vx - sin th vy, sin th vx + cos th vy), T = period_steps dt,
 * moving = (vx != 0 || vy != 0), every product and sum one rounded fp64 operation in the order written, a heading psi0 + wz (j dt) computed as psi0 + (wz j) dt:
 *   p_0 = x0[3:5];  p_{k+1} = p_k + v_w(psi0 + wz (k + 1/2) dt) dt, k = 0 ... N - 1   (a serial sum, the heading at the middle of the step)
 *   x_ref[k][2]    = psi0 + wz (k + 1) dt          (not wrapped: the plant and the solver carry unwrapped yaw)
 *   x_ref[k][3:5]  = p_{k+1} when moving, else com_target[0:2]   (a robot that turns on the spot turns about its target)
 *   x_ref[k][5]    = com_target[2];  x_ref[k][8] = wz;  x_ref[k][9:11] = v_w(psi0 + wz (k + 1) dt);  x_ref[k][12] = x0[12];  every other entry 0
 *   pcom[k]        = (p_k, x0[5]);   foot: the current contact points repeated;   contact: the schedule of srbdqp_mpc_inputs_*
 *   psi_L          = psi0 + wz (T / 2)             (the heading at mid-swing)
 *   landing_xy     = ((x0[3:5] + Rz(psi_L) (0, side hip_offset_y)) + (T / 2) x0[9:11]) + 0.03 (x0[9:11] - v_w(psi0)),  side as in srbdqp_mpc_inputs_*
 *   landing_z      = 0;   landing_yaw = psi_L
 * The host form refuses a command that is not finite (SRBDQP_E_INVALID).  In the device form such a command gives references that are not numbers for that
 * robot alone, which its solve answers with status -1 and zero forces (srbdqp.h, the non-finite contract); no trip count depends on a command.
 * Any horizon of the handle, live ones included.  srbdqp_kernel_name: mpc_inputs_steered_f64. */
int srbdqp_mpc_inputs_steered_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                  const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                  double* landing, double* landing_yaw);
int srbdqp_mpc_inputs_steered_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                         const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                         double* landing, double* landing_yaw, void* stream);

/* srbdqp_fleet_advance_* with landing_yaw [B] (required), as srbdqp_mpc_inputs_steered_* wrote it.  One thing differs, the touchdown:
 *   heel = landing - foot_half_length (cos psi_L, sin psi_L, 0),  toe = landing + foot_half_length (cos psi_L, sin psi_L, 0)
 * z on flat ground is landing's z; with a map set each of the two turned points gets z = S(own xy).z.  landing_yaw = 0 is srbdqp_fleet_advance_* bit for bit.
 * srbdqp_kernel_name: fleet_advance_steered_f64, fleet_advance_terrain_steered_f64. */
int srbdqp_fleet_advance_steered_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                                     const double* landing, const double* landing_yaw, const uint8_t* standing, const double* push, uint8_t* alive,
                                     const srbdqp_fleet_settings* cfg);
int srbdqp_fleet_advance_steered_device_f64(srbdqp_handle* h, int64_t B, double* x, double* feet, double* stamp, const double* u0, int64_t u0_stride,
                                            const double* landing, const double* landing_yaw, const uint8_t* standing, const double* push, uint8_t* alive,
                                            const srbdqp_fleet_settings* cfg, void* stream);

/* The roll-out under commands: the loop of srbdqp_fleet_rollout_* with srbdqp_mpc_inputs_steered_device_f64 as its inputs call and the steered plant step, a
 * landing_yaw buffer joining the handle's roll-out allocation.  The arguments of srbdqp_fleet_rollout_observed_* with command and command_steps in place of v_ref:
 *   command_steps == 1: command [B][3], held over the call;  command_steps == T: command [T][B][3], step t reading row t.
 *   obs == NULL: the plain loop (w_est and w_log are ignored);  obs != NULL: the observed loop;  a terrain set on the handle: the terrain roll-out.
 * Refused: what the roll-out it becomes refuses; command NULL; command_steps outside {1, T}; in the host form a command that is not finite.  Chunks compose bit
 * for bit, a schedule with the two constant-command chunks it is made of included.
 * Not modelled: a centrifugal term in the landing point, feet turned under a standing robot, ragged fleets, fp32.  foot[b][k] stays the current points along
 * the horizon; srbdqp_fleet_rollout_previewed_* below previews the footholds.  (A robot that is to be where its commands lead: srbdqp_fleet_rollout_tracked_* below.) */
int srbdqp_fleet_rollout_steered_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                            int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                            double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                            const srbdqp_observer_settings* obs, double* w_est, double* w_log, void* stream);
int srbdqp_fleet_rollout_steered_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                     int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                     double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                     const srbdqp_observer_settings* obs, double* w_est, double* w_log);

/* ---- a fleet that follows its path: a carried reference pose with a bounded lead.
 *
 * srbdqp_mpc_inputs_steered_* restarts its references from the measured state at every control step, so a lag behind the command is never integrated away.  A
 * tracked robot has a pose (qx, qy, th) -- a planar reference position and an unwrapped reference heading -- in a caller-owned array pose [B][3] that goes in
 * and out, the way w_est does for the observer: the references start from the pose, the pose moves on with the command, and a bound keeps it from running
 * ahead of a robot that is held back.  srbdqp_mpc_inputs_tracked_* per robot, with the command (vx, vy, wz), psi0 = x0[2], and v_w, the heading psi + (wz j) dt,
 * the table of positions and T = period_steps dt as in srbdqp_mpc_inputs_steered_*; every product and sum one rounded fp64 operation in the order written:
 *   1. bound     dx = qx - x0[3];  dy = qy - x0[4];  n = sqrt(dx dx + dy dy)
 *                if n > lead_max:  s = lead_max / n;  qx = x0[3] + dx s;  qy = x0[4] + dy s
 *                dth = th - psi0;  if dth > yaw_lead_max: th = psi0 + yaw_lead_max;  else if dth < -yaw_lead_max: th = psi0 - yaw_lead_max
 *                A pose inside the bounds is untouched, bit for bit.  Every comparison is false on a NaN: a state or a pose that is not finite clamps nothing.
 *   2. refer     q_0 = (qx, qy);  q_{k+1} = q_k + v_w(th + wz (k + 1/2) dt) dt, k = 0 ... N - 1   (the serial sum of the steered call, from the pose)
 *                x_ref[k][2]    = th + (wz (k + 1)) dt
 *                x_ref[k][3:5]  = q_{k+1}, moving or not: a zero planar velocity holds the pose's position, it does not go back to com_target
 *                x_ref[k][5]    = com_target[2];  x_ref[k][8] = wz;  x_ref[k][9:11] = v_w(th + (wz (k + 1)) dt);  x_ref[k][12] = x0[12];  every other entry 0
 *   3. measured  pcom, foot, contact, landing and landing_yaw are those of srbdqp_mpc_inputs_steered_*, bit for bit: the linearisation points and the Raibert
 *                landing point belong to where the robot is.
 *   4. advance   pose' = (q_1, th + (wz 1) dt).  If one of the three is not finite the pose is written back as it stood after step 1: a bad command row costs
 *                that robot one step, not the rest of the roll-out.  (The references of that step are not numbers, and the solve's non-finite contract
 *                answers them as in the steered call.)
 * With pose = (x0[3], x0[4], x0[2]) and a moving command every output is srbdqp_mpc_inputs_steered_*'s bit for bit.  The host forms refuse a pose or a command
 * that is not finite, by robot (SRBDQP_E_INVALID); the device forms follow the rules above, and no trip count depends on a command, a state or a pose.  Any
 * horizon of the handle, live ones included.  srbdqp_kernel_name: mpc_inputs_tracked_f64. */
typedef struct srbdqp_track_settings {
    int32_t struct_size;          /* = sizeof(srbdqp_track_settings) */
    int32_t reserved0;
    double lead_max;              /* how far the pose's position may lie from the measured one, m: finite, positive (0.1) */
    double yaw_lead_max;          /* how far its heading may lie from the measured yaw, rad: finite, positive (0.3) */
} srbdqp_track_settings;

/* The defaults above into *s; s->struct_size says how large the caller's struct is (checked before anything is written). */
int srbdqp_track_default_settings(srbdqp_track_settings* s);

/* The arguments of srbdqp_mpc_inputs_steered_*, then trk and pose [B][3] in/out (required). */
int srbdqp_mpc_inputs_tracked_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                  const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                  double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose);
int srbdqp_mpc_inputs_tracked_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                         const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                         double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose, void* stream);

/* srbdqp_fleet_rollout_steered_* with srbdqp_mpc_inputs_tracked_device_f64 as its inputs call; nothing else in the loop changes, so a terrain on the handle,
 * obs != NULL and the plain loop work as they do there.  The arguments of the steered roll-out, then trk, pose [B][3] in/out (required) and pose_log [T][B][3]
 * or NULL: pose_log[t] is the pose behind step t, written by the inputs kernel itself (no further launch).
 * Refused: what the roll-out it becomes refuses; pose NULL; bad track settings; in the host form a pose or a command that is not finite, by robot.  Chunks
 * compose bit for bit with pose carried by the caller, a schedule with its constant-command chunks included.
 * A robot that has fallen holds its state while its pose keeps moving on and keeps being clamped to within the bounds of that held state.
 * Not modelled: ragged fleets, fp32, a pose for the unsteered v_ref roll-out.  (Footholds previewed along the horizon: srbdqp_fleet_rollout_previewed_* below.) */
int srbdqp_fleet_rollout_tracked_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                            int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                            double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                            const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                            const srbdqp_track_settings* trk, double* pose, double* pose_log, void* stream);
int srbdqp_fleet_rollout_tracked_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                     int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                     double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                     const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                     const srbdqp_track_settings* trk, double* pose, double* pose_log);

/* ---- a fleet that previews its footholds along the horizon.
 *
 * srbdqp_mpc_inputs_steered_* and ..._tracked_* write the contact schedule of the whole horizon but foot[b][k] = feet[b] at every k: a foot that lands inside
 * the horizon is given its force at the old point.  The previewed call moves the plant's own touchdown rule along the horizon.  Every product and sum is one
 * rounded fp64 operation in the order written, no fused multiply-add.  With P = period_steps, ds = double_support_steps, p0 the phase of step 0 in [0, 2 P)
 * (the step index floor(stamp / dt + 1e-9) mod 2 P), flag_f(k) the stance flag of foot f -- the left (contacts 0, 1) or the right (contacts 2, 3) -- at step k:
 *   touchdown  of f at step j: 1 <= j <= N - 1, flag_f(j - 1) == 0 and flag_f(j) == 1.  In closed form: the left foot lands where (p0 + j) mod 2 P == 0, the
 *              right foot where (p0 + j) mod 2 P == P; the latest touchdown step j <= k is j = k - ((p0 + k) mod 2 P) for the left foot and
 *              j = k - ((p0 + k + P) mod 2 P) for the right, a touchdown where j >= 1.  A standing robot, ds >= P and N = 1 have none; at most one foot lands at a step.
 *   state      behind step j - 1, where the inputs call of that later step would compute `landing` if the robot sat on its own measured-state table:
 *              j - 1 = 0: the measured x0: heading x0[2], position x0[3:5], velocity x0[9:11], the command's velocity v_w(psi0 + (wz 0) dt);
 *              j - 1 >= 1: heading psi0 + (wz (j - 1)) dt, position p_{j-1} of srbdqp_mpc_inputs_steered_*'s table (the measured state's, in tracked calls
 *              too), velocity v_w at that heading, which is the command's velocity as well: the 0.03 feedback term is an exact zero for finite inputs.
 *   foothold   psi_L,j = heading + wz (T / 2);  (lx, ly) = landing_xy of srbdqp_mpc_inputs_steered_* at that state, side that of the foot that lands;
 *              heel = (lx, ly) - foot_half_length (cos psi_L,j, sin psi_L,j),  toe = (lx, ly) + foot_half_length (cos psi_L,j, sin psi_L,j);  z = 0.
 *   foot[b][k] for the contacts of f: heel and toe of the latest touchdown j <= k of f, the current points where there is none (a swing foot keeps its last
 *              point until it lands, as before).
 *   previewed  [B][N][4] uint8, may be NULL: 1 where foot[b][k] holds a previewed point for that contact.
 * x_ref, pcom, contact, landing, landing_yaw and the pose are those of the steered or tracked call, bit for bit.  For a touchdown at j = 1 heel and toe are, bit for
 * bit, what srbdqp_fleet_advance_steered_* writes from this call's landing and landing_yaw with the same foot_half_length, and psi_L,1 == landing_yaw: the
 * foothold solve t assumes at horizon step 1 is the one solve t + 1 finds at step 0.  A command or a state that is not finite spoils the rows of that robot
 * alone; no trip count, index or branch depends on a command, a state or a pose.
 * srbdqp_kernel_name: mpc_inputs_previewed_f64, mpc_inputs_tracked_previewed_f64, terrain_inputs_previewed_f64. */
typedef struct srbdqp_preview_settings {
    int32_t struct_size;          /* = sizeof(srbdqp_preview_settings) */
    int32_t reserved0;
    double foot_half_length;      /* heel and toe lie this far behind and ahead of the landing point: the plant's srbdqp_fleet_settings value (0.085) */
} srbdqp_preview_settings;

/* The defaults above into *s; s->struct_size says how large the caller's struct is (checked before anything is written). */
int srbdqp_preview_default_settings(srbdqp_preview_settings* s);

/* The arguments of srbdqp_mpc_inputs_tracked_*, then prv and previewed.  trk == NULL: the steered form (pose is ignored); trk != NULL: the tracked form.
 * Refused: what that form refuses; a wrong struct_size of prv; a foot_half_length that is not finite and positive. */
int srbdqp_mpc_inputs_previewed_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                    const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                    double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose,
                                    const srbdqp_preview_settings* prv, uint8_t* previewed);
int srbdqp_mpc_inputs_previewed_device_f64(srbdqp_handle* h, int64_t B, const double* x0, const double* feet, const double* stamp, const double* command,
                                           const uint8_t* standing, const srbdqp_gait* gait, double* x_ref, double* foot, uint8_t* contact, double* pcom,
                                           double* landing, double* landing_yaw, const srbdqp_track_settings* trk, double* pose,
                                           const srbdqp_preview_settings* prv, uint8_t* previewed, void* stream);

/* srbdqp_terrain_inputs_* under footholds that differ from step to step: foot [B][N][12] in/out and previewed [B][N][4] (may be NULL: none) as
 * srbdqp_mpc_inputs_previewed_* wrote them, x_ref [B][N][13] in/out, normals [B][N][12] out.  For every (b, k, i): normals[b][k][i] = S(xy of foot[b][k][i]).n; a
 * previewed point gets z = S(own xy).z, the plant's touchdown rule, and any other point keeps its z; x_ref[b][k][5] += (((z0 + z1) + z2) + z3) 0.25 over the z of
 * foot[b][k] after that write: the height reference follows the ground the robot will stand on at step k.  With previewed all zero the outputs are those of
 * srbdqp_terrain_inputs_* on foot[b][0], bit for bit.  Without a map: SRBDQP_E_INVALID. */
int srbdqp_terrain_inputs_previewed_f64(srbdqp_handle* h, int64_t B, double* foot, const uint8_t* previewed, double* x_ref, double* normals);
int srbdqp_terrain_inputs_previewed_device_f64(srbdqp_handle* h, int64_t B, double* foot, const uint8_t* previewed, double* x_ref, double* normals, void* stream);

/* The steered roll-out -- with trk != NULL the tracked one -- whose inputs call is srbdqp_mpc_inputs_previewed_device_f64 and which on a terrain enqueues
 * srbdqp_terrain_inputs_previewed_device_f64 in place of srbdqp_terrain_inputs_device_f64, a previewed buffer joining the handle's roll-out allocation.  Nothing
 * else in the loop changes: the solve, the plant, the gait and the observer are those of srbdqp_fleet_rollout_steered_*.  The arguments of the tracked
 * roll-out, then prv; with trk == NULL pose and pose_log are ignored.
 * Refused: what the roll-out it becomes refuses; bad preview settings; a prv->foot_half_length that differs from cfg->foot_half_length (the MPC would preview
 * another foot than the plant puts down).  Chunks compose bit for bit.
 * Not modelled: a preview for the v_ref roll-out, ragged fleets, fp32, feet turned under a standing robot, a centrifugal term in the landing point. */
int srbdqp_fleet_rollout_previewed_device_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                              int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                              double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                              const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                              const srbdqp_track_settings* trk, double* pose, double* pose_log, const srbdqp_preview_settings* prv, void* stream);
int srbdqp_fleet_rollout_previewed_f64(srbdqp_handle* h, int64_t B, int32_t T, double* x, double* feet, double* stamp, const double* command,
                                       int32_t command_steps, const uint8_t* standing, const double* push, const srbdqp_fleet_settings* cfg, uint8_t* alive,
                                       double* x_log, double* u0_log, double* feet_log, int32_t* status_log, int32_t* iters_log,
                                       const srbdqp_observer_settings* obs, double* w_est, double* w_log,
                                       const srbdqp_track_settings* trk, double* pose, double* pose_log, const srbdqp_preview_settings* prv);

#ifdef __cplusplus
}
#endif
#endif /* SRBDQP_CASCADE_H */
