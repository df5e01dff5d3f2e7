/*
 * cmpc_rbd.h -- C ABI of the batched rigid-body model (libcmpc_amd.so): what the whole-body QP of include/cmpc_wbc.h and
 * the gain tracking of include/cmpc.h take from a rigid-body library in the reference (DART, code/inverse_dynamics.py:46-65,
 * :112, :116 and code/simulation.py:303-388), for B robots in one launch.
 *
 * The model is a kinematic tree of 25 bodies: body 0 is the floating base, body i (1..24) hangs on body parent[i] < i by a
 * one-dof revolute joint and is moved by dof 5 + i.  Fixed joints are merged by the caller (cmpc_amd/rbd.py).  Host tables
 * of cmpc_rbd_model_create, all row-major, entry 0 of the joint tables unused:
 *   parent     [25]      parent[0] = -1, 0 <= parent[i] < i
 *   joint_R    [25][9]   rotation parent body <- joint frame at angle 0 (orthonormal)
 *   joint_p    [25][3]   joint origin in the parent body
 *   axis       [25][3]   joint axis in the joint frame (finite, non-zero; normalised here)
 *   mass       [25]      >= 0, total > 0
 *   com        [25][3]   centre of mass in the body frame
 *   inertia    [25][6]   rotational inertia about the centre of mass, body axes: xx xy xz yy yz zz
 *   frame_body [4]       body of the task frames lfoot, rfoot, torso, base
 *   frame_R    [4][9]    rotation body <- frame       frame_p [4][3]  frame origin in the body
 * Everything is validated on the host, so that no table can index outside the kernel's arrays.
 *
 * Coordinates: q[0:3] rotation vector of the base (world <- base), q[3:6] base origin in the world, q[6+k] joint angles;
 * v[0:3] base angular and v[3:6] base-origin linear velocity in the BASE frame (the body twist), v[6+k] joint rates.
 * M and h are those of  M vdot + h = S' tau + Jc' f  with vdot the plain time derivative of v and gravity (0, 0, -g).
 *
 * cmpc_rbd_eval: DEVICE pointers, instance-major; any output may be NULL (skipped).
 *   q, v     [B][30]
 *   J        [B][21][30]  task Jacobian, rows of CMPC_WBC_TASK_ROWS: lfoot angular 3 + linear 3 (sole origin, world),
 *                         rfoot 6, com linear 3, torso angular 3, base angular 3
 *   jdqd     [B][21]      classical bias acceleration Jdot v of those rows
 *   M        [B][30][30]  mass matrix, bit-for-bit symmetric        h [B][30]  Coriolis + centrifugal + gravity
 *   pose     [B][21]      foot rotation vector 3 + position 3 (twice), com 3, torso rotation vector 3, base rotation vector 3
 *   vel      [B][21]      J v
 *   centroid [B][9]       com, com velocity, angular momentum about the com (world): columns 0..8 of the MPC's x0
 * A row of q or v with a non-finite word makes that instance's outputs NaN and touches no other instance.
 * Asynchronous on `stream` (hipStream_t; NULL = default stream); allocates nothing; no host synchronisation.
 * Returns 0 on success; message via cmpc_rbd_last_error.
 *
 * cmpc_rbd_eval_inertial: the same contract for a fleet whose robots carry their own inertial parameters (a payload, a
 * domain-randomised batch).  Kinematics, frames and topology are the model's; mass, centre of mass and inertia of body i of
 * robot b are the CMPC_RBD_INERTIAL_WORDS words of
 *   inertial [B][25][10]  DEVICE pointer: mass, com x y z, inertia xx xy xz yy yz zz -- the host tables' words, same meaning
 * and the total mass of robot b is its row's masses summed in body order 0 .. 24.  The table is read at every launch, so a
 * caller may rewrite rows between launches (a robot picks a box up or drops it).  A row with a non-finite word, a mass < 0
 * or a total that is not finite and > 0 makes that instance's outputs NaN, as a non-finite q does, and touches no other
 * instance; that an inertia is positive definite is not checked, as on the host.  A null `inertial` is refused.
 */
#ifndef CMPC_RBD_H
#define CMPC_RBD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMPC_RBD_BODIES 25
#define CMPC_RBD_DOFS 30   /* CMPC_WBC_DOFS */
#define CMPC_RBD_FRAMES 4
#define CMPC_RBD_ROWS 21   /* CMPC_WBC_TASK_ROWS */
#define CMPC_RBD_INERTIAL_WORDS 10

typedef struct cmpc_rbd_model cmpc_rbd_model;

int cmpc_rbd_model_create(int device, const int32_t *parent, const double *joint_R, const double *joint_p, const double *axis,
                          const double *mass, const double *com, const double *inertia, const int32_t *frame_body,
                          const double *frame_R, const double *frame_p, cmpc_rbd_model **out);
int cmpc_rbd_model_destroy(cmpc_rbd_model *model);

int cmpc_rbd_eval(const cmpc_rbd_model *model, int32_t B, const double *q, const double *v, double g, double *J, double *jdqd,
                  double *M, double *h, double *pose, double *vel, double *centroid, void *stream);
int cmpc_rbd_eval_inertial(const cmpc_rbd_model *model, int32_t B, const double *q, const double *v, const double *inertial,
                           double g, double *J, double *jdqd, double *M, double *h, double *pose, double *vel, double *centroid,
                           void *stream);

const char *cmpc_rbd_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* CMPC_RBD_H */
