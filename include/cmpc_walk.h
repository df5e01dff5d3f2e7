/*
 * cmpc_walk.h -- C ABI of the walking loop around the batched rigid-body model (libcmpc_amd.so): the whole-body task
 * references of B robots from each robot's own adapted plan (code/simulation.py:227-231, :269-271 and
 * code/inverse_dynamics.py:68-89 of the reference), the step that advances (q, v) by the whole-body QP's acceleration, the
 * measurement that feeds the robot back to its MPC and the contact plant that moves it by torques, ground and pushes, one
 * launch each.  Coordinates and task rows are those of include/cmpc_rbd.h and include/cmpc_wbc.h.
 *
 * cmpc_walk_gait_create: HOST tables of S walks, row-major, padded per scene (padding is never read):
 *   T          [S]                  ticks of each scene, 1 <= T[s] <= T_max
 *   step_idx   [S][T_max]           step index at every tick, 0 <= step_idx < n_steps[s]
 *   n_steps    [S]                  plan entries, 1 <= n_steps[s] <= n_steps_max
 *   step_start [S][n_steps_max]     first tick of each step; step_start[step_idx[t]] <= t
 *   ss_dur     [S][n_steps_max]     single-support ticks, > 0 (entry 0, the initial double support: >= 0)
 *   support_l  [S][n_steps_max]     uint8, 1 where the support foot is the left one
 *   ang        [S][n_steps_max][3]  orientation of each plan entry (finite)
 *   init_feet  [S][12]              initial lfoot, rfoot poses as [ang, pos] (finite)
 *   step_height, delta              swing apex; the world time step, > 0
 * Everything is validated on the host, so that no entry can index outside an array.
 *
 * cmpc_walk_task_refs: DEVICE pointers, instance-major.
 *   t [B] int32, scene_id [B] int32 (NULL = scene 0)
 *   plan_pos [B][n_steps_max][3]    the plan cmpc_rollout_advance writes
 *   pose, vel, jdqd [B][21]         of cmpc_rbd_eval            com_des [B][9]  desired CoM position, velocity, acceleration
 *   q, v [B][30]                    q_ref [30]  the posture the joint task holds (NULL = zeros); its velocity is 0
 *   ff, pos_err, vel_err [B][51]    the inputs of cmpc_wbc_qp_solve_tasks with Jdot = NULL (-jdqd folded into ff)
 *   feet_des [B][36]                lfoot [ang, pos] 6, velocity 6, acceleration 6; then rfoot
 * Any output may be NULL (skipped).  The desired feet are the swing-foot generator's on the robot's own plan; torso and
 * base follow the mean of the feet's first three entries; angular position errors are Log(R_des R_cur'), world frame;
 * rows 21..26 (the base dofs of the joint task) are 0.  A robot whose scene_id is outside [0, S), whose t is outside
 * [0, T[s]), whose step_idx + 1 >= n_steps[s], or with a non-finite word in an input row (of plan_pos: the entries in use)
 * gets NaN in every output and touches no other robot; the checks are made before any table is read with that index.
 *
 * cmpc_walk_integrate: DEVICE pointers.  With R = Exp(q[0:3]):
 *   v+ = v + dt qdd;  R+ = R Exp(dt v+[0:3]);  p+ = p + dt R v+[3:6];  q+[0:3] = Log(R+), angle <= pi;  q+[6:] = q[6:] + dt v+[6:]
 * A robot with hold[b] != 0 (hold may be NULL) or a non-finite word in q, v or qdd keeps (q, v) bit for bit.
 * q_out == q and v_out == v (in place) are allowed.
 *
 * cmpc_walk_measure: DEVICE pointers, instance-major: the measured x_0 of the MPC (code/simulation.py:201-204 and
 * code/centroidal_mpc_vertices.py:482-489 of the reference) from the robot's own evaluation.
 *   centroid [B][9], pose [B][21]   of cmpc_rbd_eval
 *   state [B][16]                   the rollout's [com dcom hw theta_hat yaw_l yaw_r mass mu], updated in place
 *   alive [B] uint8                 updated in place (NULL: every robot counts as alive, nothing is written)
 *   x_meas [B][20], innovation [B][9]   optional outputs (NULL = skipped)
 * Per robot, every input is read before any word is written.  dead = alive && alive[b] == 0; bad = a non-finite word among
 * the 30 of centroid[b] and pose[b]; fallen = !(centroid[b][2] > z_min) || !(R22 > cos_tilt_min), R22 the last entry of
 * Exp(pose[b][18:21]), the cosine of the base's tilt from the vertical (-INFINITY disables a guard).
 *   dead             state[b], alive[b] keep their bits; the rows of x_meas and innovation are NaN
 *   bad or fallen    state[b] keeps its bits, alive[b] = 0; both rows are NaN
 *   otherwise        innovation[b] = centroid[b] - state[b][0:9] (measured minus predicted, from the old state);
 *                    state[b][0:9] = centroid[b]; state[b][12] = pose[b][2]; state[b][13] = pose[b][8] (the third angle of
 *                    each foot pose); theta_hat, mass and mu are not touched;
 *                    x_meas[b] = [centroid 9, state[9:12], pose[2], pose[3], pose[4], 0, pose[8], pose[9], pose[10], 0],
 *                    the x_meas of cmpc_gain_track
 * No robot's row touches another robot's.  B < 0, a NaN z_min or cos_tilt_min and a null centroid, pose or state are refused.
 *
 * cmpc_walk_plant_step: DEVICE pointers, instance-major: the contact plant.  Joint torques, a wrench on the base and a flat
 * frictional floor under the eight sole vertices move the robot one tick (what the reference leaves to DART's world step,
 * code/simulation.py:193-300): a velocity-level time-stepping scheme, the contact impulses by projected Gauss-Seidel.
 *   q, v [B][30]; M [B][30][30], h [B][30], J [B][21][30], pose [B][21]   of cmpc_rbd_eval at that same (q, v)
 *   tau       word j of row b (leading dimension tau_ld >= 24) is the torque of dof 6 + j; NULL = zero torques
 *   ext [B][6]        world-frame moment, then world-frame force at the base origin; NULL = none.  With R = Exp(q[0:3]) the
 *                     generalised force is [R'm; R'f; 0]
 *   foot_mu [B][2]    half foot size d and the floor's friction mu (the layout of cmpc_wbc_qp_solve_tasks)
 *   hold [B] uint8    may be NULL
 *   impulse [B][24]   in/out: last tick's impulses as the warm start, written with this tick's (world x, y, z per vertex,
 *                     N s); NULL = cold start, nothing returned
 *   q_out, v_out [B][30] (== q, v allowed); status [B] int32 and residual [B] are optional (NULL = skipped)
 * Vertex i = 4f + k belongs to foot f (0 left, 1 right); corner k has the signs (sx, sy) = (+,+), (+,-), (-,+), (-,-).
 *   R_f = Exp(pose[6f:6f+3]);  p_f = pose[6f+3:6f+6];  r_i = R_f (sx d, sy d, 0);  phi_i = (p_f + r_i).z - ground_z
 *   Jc[3i:3i+3] = J[6f+3:6f+6] - [r_i]x J[6f:6f+3]
 *   v_free = v + dt M^-1 ([R'm; R'f; tau] - h);   Y = M^-1 Jc';   W = Jc Y + cfm I
 *   c = Jc v_free;   c[3i+2] += (phi_i >= 0 ? phi_i : erp phi_i) / dt
 *   p = the warm start made admissible: p_n <- max(0, p_n), then (p_x, p_y) scaled onto the disk of radius mu p_n
 *   `sweeps` times, i = 0..7 in order:  p_n <- max(0, p_n - (W[n].p + c_n) / W[n][n]) for n = 3i+2;
 *       p_a <- p_a - (W[a].p + c_a) / W[a][a] for a = 3i, 3i+1 (each with the p just updated);
 *       (p_x, p_y) scaled onto the disk of radius mu p_n (to 0 when p_n = 0)
 *   v+ = v_free + Y p;   q+ from (q, v+, dt) as in cmpc_walk_integrate
 * All eight vertices are always in the problem; the cone is the circular one; the sweep count is fixed.
 *   status 0  stepped
 *          1  held (hold[b] != 0): (q, v) keep their bits, the rows of impulse and residual are not touched
 *          2  refused: (q, v) keep their bits, the impulse row is zeros, residual is NaN -- a non-finite word in an input
 *             row of the robot (the warm start included), a foot_mu entry that is not finite and > 0, or a Cholesky pivot
 *             of M that is not finite and > 0
 *   residual  max_i max(0, -(W p + c)[3i+2]) after the last sweep: the normal velocity, in m/s, by which the step still
 *             violates non-penetration
 * Per robot every input is read before any word is written, and no robot's row touches another robot's.  Refused before the
 * launch: B < 0; a null q, v, M, h, J, pose, foot_mu, q_out, v_out or params; tau_ld < 24; sweeps < 0; dt not finite and
 * > 0; erp outside [0, 1]; cfm < 0; a non-finite ground_z; a wrong struct_size.
 * cmpc_walk_plant_default_params: struct_size, sweeps = 50, dt = 0.01, ground_z = 0, erp = 0.2, cfm = 0.  These are starting
 * values, NOT validated ones: on a standing HRP-4 from a cold start 30 sweeps leave |v+| at 2.7e-2, 100 at 5e-4; read
 * `residual`.
 *
 * The launches are asynchronous on `stream` (hipStream_t; NULL = default stream), allocate nothing and do not synchronise
 * the host.  Every function returns 0 on success; message via cmpc_walk_last_error.
 */
#ifndef CMPC_WALK_H
#define CMPC_WALK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMPC_WALK_ROWS 51        /* CMPC_WBC_TASK_ROWS + CMPC_WBC_DOFS */
#define CMPC_WALK_FEET_WORDS 36

typedef struct cmpc_walk_gait cmpc_walk_gait;

int cmpc_walk_gait_create(int device, int32_t S, int32_t T_max, int32_t n_steps_max, const int32_t *T, const int32_t *step_idx,
                          const int32_t *n_steps, const int32_t *step_start, const int32_t *ss_dur, const uint8_t *support_l,
                          const double *ang, const double *init_feet, double step_height, double delta, cmpc_walk_gait **out);
int cmpc_walk_gait_destroy(cmpc_walk_gait *gait);

int cmpc_walk_task_refs(const cmpc_walk_gait *gait, int32_t B, const int32_t *t, const int32_t *scene_id, const double *plan_pos,
                        const double *pose, const double *vel, const double *jdqd, const double *com_des, const double *q,
                        const double *v, const double *q_ref, double *ff, double *pos_err, double *vel_err, double *feet_des,
                        void *stream);

int cmpc_walk_integrate(int device, int32_t B, const double *q, const double *v, const double *qdd, double dt,
                        const uint8_t *hold, double *q_out, double *v_out, void *stream);

int cmpc_walk_measure(int device, int32_t B, const double *centroid, const double *pose, double z_min, double cos_tilt_min,
                      double *state, uint8_t *alive, double *x_meas, double *innovation, void *stream);

typedef struct cmpc_walk_plant_params {
  int32_t struct_size, sweeps;     /* sizeof(cmpc_walk_plant_params); Gauss-Seidel sweeps over the eight vertices */
  double dt, ground_z, erp, cfm;   /* time step; floor height; share of a penetration removed per tick; W's diagonal term */
} cmpc_walk_plant_params;

void cmpc_walk_plant_default_params(cmpc_walk_plant_params *p);

int cmpc_walk_plant_step(int device, int32_t B, const double *q, const double *v, const double *M, const double *h,
                         const double *J, const double *pose, const double *tau, int32_t tau_ld, const double *ext,
                         const double *foot_mu, const uint8_t *hold, const cmpc_walk_plant_params *params,
                         double *impulse, double *q_out, double *v_out, int32_t *status, double *residual, void *stream);

const char *cmpc_walk_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* CMPC_WALK_H */
