/*
 * cmpc_wbc.h -- C ABI of the batched whole-body inverse-dynamics QP (libcmpc_amd.so), SURVEY.md 8f row 4.
 *
 * Replaces, for B robots at once, the QP that the reference assembles and hands to CasADi's conic interface / OSQP
 * once per simulator tick:
 *   code/inverse_dynamics.py:92-105   cost          1/2 qdd' Hq qdd + Fq' qdd + 1/2 1e-6 |f_c|^2  (Hq, Fq: task sums)
 *   code/inverse_dynamics.py:107-111  dynamics      M qdd + h - Jc' f_c = S tau,  S = blockdiag(0_6, I)
 *   code/inverse_dynamics.py:113-129  inequalities  8 CoP / friction rows per foot wrench, d = foot_size / 2, mu
 *   code/inverse_dynamics.py:131-134  qp_solver.set_values(...); solve(); tau = solution[tau_indices]; return tau[6:]
 *   code/utils.py:40-92               QPSolver (Opti('conic') + OSQP)
 * The reference has no native interface here either (CasADi's SWIG layer); this header is what a ctypes stub binds
 * (INTEGRATION.md).  Sizes are the reference's for HRP-4: 30 dofs (6 floating-base), two 6-D contact wrenches.
 * Every pointer is a DEVICE pointer owned by the caller; matrices are row-major, instance-major:
 *   Hq [B][30][30]  Fq [B][30]   task Hessian / gradient in qdd (symmetric positive definite)
 *   M  [B][30][30]  h  [B][30]   mass matrix, Coriolis + gravity forces
 *   Jc [B][12][30]               contact Jacobian, rows already scaled by the contact flags (:109)
 * Outputs: tau [B][30] (tau[0:6] = 0: the statement leaves them free and the reference discards them), qdd [B][30],
 * f_c [B][12], status [B] (0 = KKT error <= tol, 1 = iteration cap, 2 = numerical failure; for 1 and 2 tau, qdd and f_c are
 * ZEROS, the reference's QPSolver.solve on failure, code/utils.py:85-92), iters [B].
 * Asynchronous on `stream` (hipStream_t; NULL = default stream).  Returns 0 on success; message via cmpc_wbc_last_error.
 */
#ifndef CMPC_WBC_H
#define CMPC_WBC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMPC_WBC_DOFS 30
#define CMPC_WBC_BASE 6
#define CMPC_WBC_CONTACT 12
#define CMPC_WBC_INEQ 16
#define CMPC_WBC_TASK_ROWS 21 /* lfoot 6, rfoot 6, com 3, torso 3, base 3: the Jacobians of :46-51, stacked in that order */
#define CMPC_WBC_NACC (CMPC_WBC_TASK_ROWS + CMPC_WBC_DOFS) /* 51: the 21 task rows, then the 30 rows of the joint task */

/* weights and gains of the six tasks, in the order lfoot, rfoot, com, torso, base, joints (:41-44) */
typedef struct cmpc_wbc_gains {
  int32_t struct_size, reserved; /* struct_size = sizeof(cmpc_wbc_gains), checked by the entry point */
  double weight[6], pos_gain[6], vel_gain[6];
} cmpc_wbc_gains;

int cmpc_wbc_qp_solve_batch(int device, int32_t B, const double *Hq, const double *Fq, const double *M, const double *h,
                            const double *Jc, double half_foot_size, double mu, double tol, int32_t max_iter,
                            double *tau, double *qdd, double *f_c, int32_t *status, int32_t *iters, void *stream);

/* The literals of code/inverse_dynamics.py:42-44 (and struct_size). */
void cmpc_wbc_default_gains(cmpc_wbc_gains *g);

/*
 * The same QP from the task form of code/inverse_dynamics.py:46-103, with the parameters of instance b in row b:
 *   J        [B][21][30]  task Jacobians (:46-51), rows lfoot 6, rfoot 6, com 3, torso 3, base 3
 *   Jdot     [B][21][30]  their derivatives (:60-64); NULL = the caller folded -Jdot qd into acc_ff (qd is not read then)
 *   acc_ff   [B][51]      feed-forward accelerations (:68-73): the 21 task rows, then the 30 joints
 *   pos_err  [B][51]      (:76-81)        vel_err [B][51]  (:84-89)
 *   qd       [B][30]      current['joint']['vel']
 *   joint_sel[30]         diagonal of joint_selection (:24-28), shared by the batch
 *   M, h                  as above
 *   contact  [B][2]       left, right contact flag: multiplies that foot's Jacobian rows in Jc (:114)
 *   foot_mu  [B][2]       half foot size d, friction coefficient mu of instance b
 *   gains                 HOST pointer, read before the call returns
 * Hq = sum_t w_t J_t' J_t and Fq = -sum_t w_t J_t' (ff + k_v e_v + k_p e_p - Jdot_t qd) (:98-106; the joint task adds
 * w diag(sel^2) and -w sel (ff + k_v e_v + k_p e_p)) are formed on the device, Jc = [contact_l J[0:6]; contact_r J[6:12]];
 * instance b then solves exactly the QP of cmpc_wbc_qp_solve_batch with d, mu of its row of foot_mu.  Outputs and status
 * as above.  Rows are checked on the device: a row of foot_mu that is not finite and > 0 gives status 2, iters 0 and
 * zero outputs for that instance alone; any other non-finite input ends in status 2 with zeros as well.
 * Asynchronous on `stream`; allocates nothing (capturable in a HIP graph).
 */
int cmpc_wbc_qp_solve_tasks(int device, int32_t B, const double *J, const double *Jdot, const double *acc_ff,
                            const double *pos_err, const double *vel_err, const double *qd, const double *joint_sel,
                            const double *M, const double *h, const double *contact, const double *foot_mu,
                            const cmpc_wbc_gains *gains, double tol, int32_t max_iter, double *tau, double *qdd,
                            double *f_c, int32_t *status, int32_t *iters, void *stream);
const char *cmpc_wbc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* CMPC_WBC_H */
