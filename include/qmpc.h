/*
 * qmpc.h -- C ABI of the MI355X-native batched quaternion-MPC inner loop.
 *
 * This is the drop-in boundary for ONE hot path of zixinz990/quaternion-mpc:
 * the per-tick solve inside `legged::QuatMpc::grf_update`
 * (reference legged_ctrl/src/mpc/QuatMpc.cpp:217-265: ALTRO set-up, Solve(),
 * GetInput(0)).  The reference has no FFI layer; its seam is the C++ virtual
 * class `legged::LeggedMpc` (legged_ctrl/include/mpc/LeggedMpc.h:21-28).  The
 * host-side C++ class `legged::QuatMpcHip` (quaternion-mpc_amd/host/QuatMpcHip.h)
 * keeps that virtual surface and calls the functions below instead of
 * constructing an `altro::ALTROSolver`.
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature (streams are void*)
 *   - all reals are IEEE double (the reference's a_float, QuatMpc.cpp:196)
 *     except the knot spacing, which the reference's dynamics callbacks receive
 *     as `float h` (legged_ctrl/src/utils/AltroUtils.cpp:10,79) -- kept here
 *   - quaternions are (w, x, y, z)       (QuaternionUtils.cpp:8)
 *   - 3x3 matrices are row-major; foot_pos_body is 3x4 COLUMN-major, i.e.
 *     foot_pos_body[3*leg + axis], the memory layout of the reference's
 *     Eigen::Matrix<double,3,4> (LeggedState.h:60)
 *   - leg order FL, FR, RL, RR                     (BaseInterface.cpp:11)
 *   - forces are BODY-frame, 3 per leg, as `optimized_input[0:12]`
 *     (QuatMpc.cpp:269)
 *   - nothing throws or aborts across this boundary; every entry point returns
 *     a qmpc_status and every instance gets its own status word.
 */
#ifndef QMPC_H_
#define QMPC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMPC_NX 13      /* full state  [p(3) q(4) v(3) w(3)]      QuatMpc.cpp:28  */
#define QMPC_NE 12      /* error state [dp(3) phi(3) dv(3) dw(3)] QuatMpc.cpp:212 */
#define QMPC_NU 12      /* 4 legs x (fx,fy,fz) body frame         QuatMpc.cpp:29  */
#define QMPC_NLEG 4     /* LeggedParams.h:9 */
#define QMPC_NC 24      /* friction-cone rows per knot            QuatMpc.cpp:229 */
#define QMPC_MAX_HORIZON 32

/* ---- status codes (call-level and per-instance) -------------------------- */
typedef enum qmpc_status {
  QMPC_OK = 0,              /* converged to the stated tolerances              */
  QMPC_MAX_ITER = 1,        /* iteration cap hit; forces are the last iterate
                               (this is what the reference silently returns:
                               SolveStatus ignored at QuatMpc.cpp:256)          */
  QMPC_NO_CONTACT = 2,      /* no stance leg: reference computes 0/0 at
                               QuatMpc.cpp:122; we return zero forces          */
  QMPC_NAN_INPUT = 3,       /* non-finite input record; zero forces            */
  QMPC_LINESEARCH_FAIL = 4, /* no step length reduced the merit function       */
  QMPC_NOT_PD = 5,          /* Quu lost positive definiteness                  */
  QMPC_BAD_PARAMS = 6,      /* per-instance parameter record rejected
                               (qmpc_solve_instances); zero forces             */
  /* call-level only */
  QMPC_BAD_ARGUMENT = 16,
  QMPC_NO_DEVICE = 17,      /* HIP runtime / device missing: fail loudly       */
  QMPC_HIP_ERROR = 18,
  QMPC_BATCH_TOO_LARGE = 19,
  QMPC_UNSUPPORTED = 20     /* optional dependency missing (RCCL for qmpc_gather), or a
                               call the handle does not support                 */
} qmpc_status;

/* ---- solver mode --------------------------------------------------------- */
typedef enum qmpc_mode {
  /* Converged KKT point of the NLP the reference poses (default): primal-dual
     interior point on the iLQR/Riccati core, run to tol_step / ipm_mu_final.   */
  QMPC_MODE_CONVERGED = 0,
  /* Reference-style truncated AL-iLQR: iterations_max=10, penalty_scaling=20
     (QuatMpc.cpp:22,26) and the upstream ALTRO tolerances (1e-4): the iterate the
     reference's own solver returns (status ignored, QuatMpc.cpp:256).  On the device
     for all three models.                                                       */
  QMPC_MODE_REFERENCE = 1
} qmpc_mode;

/* ---- which reference controller's inner loop ----------------------------- */
typedef enum qmpc_model {
  QMPC_MODEL_QUAT = 0,      /* legged::QuatMpc::grf_update   (QuatMpc.cpp:109-276)   */
  QMPC_MODEL_CONVEX = 1,    /* legged::ConvexMpc::grf_update (ConvexMpc.cpp:81-198):
                               12-state Euler-angle SRBD, world-frame forces    */
  QMPC_MODEL_QUAT8 = 2      /* the QuatMpc problem with 8 contact points (24 forces,
                               48 cone rows per knot): BASELINE.json config 5, the
                               SYNTHETIC stand-in for the humanoid branch that is not
                               in the reference checkout           */
} qmpc_model;

/* ---- shared, read-only problem parameters -------------------------------- */
/* Sources: legged_ctrl/config/gazebo_go1_quat_mpc.yaml:36-75,115-122 and
 * LeggedState.h:160-244 (LeggedParam). */
typedef struct qmpc_params {
  int32_t horizon;          /* N knots; param.mpc_horizon (yaml: 20)           */
  float   h;                /* knot spacing [s] AS FLOAT = (float)(mpc_update_period/1000) */
  double  h_ref;            /* knot spacing used by the reference trajectory,
                               double: i*h/1000.0 at QuatMpc.cpp:156-157       */
  double  mass;             /* param.robot_mass                                */
  double  inertia[9];       /* row-major; QuatMpc passes 1.2*trunk_inertia (QuatMpc.cpp:182) */
  double  q_weights[13];    /* diag Q on the FULL state                        */
  double  r_weights[12];    /* diag R                                          */
  double  w;                /* quaternion cost weight  w*(1-|qref'q|)          */
  double  mu;               /* friction coefficient                            */
  double  fz_max;
  int32_t mode;             /* qmpc_mode                                       */
  int32_t iterations_max;   /* both modes (reference: 10, QuatMpc.cpp:22)      */
  /* reference mode: AL-iLQR options (AltroOptions at QuatMpc.cpp:21-26 +
     upstream ALTRO defaults)                                                  */
  double  penalty_initial;
  double  penalty_scaling;
  double  penalty_max;
  double  tol_stationarity;
  double  tol_feasibility;        /* both modes (cone violation / |c+s|)       */
  double  tol_cost_intermediate;  /* dual update trigger                       */
  /* converged mode: interior-point options                                    */
  double  tol_step;               /* stop when the full Newton step |dU|_inf <=
                                     tol_step [N] ...                           */
  double  ipm_mu0;                /* initial barrier: s0=max(-c,1), lam0=mu0/s0 */
  double  ipm_mu_final;           /* ... and the barrier is <= ipm_mu_final    */
  double  ipm_sigma;              /* centering parameter                       */
  double  ipm_sigma_fast;         /* centering once full steps are taken       */
  double  ipm_tau;                /* fraction to the boundary                  */
  int32_t linesearch_max;         /* reference mode: max halvings              */
  /* parity switches for the reference's quirks */
  int32_t drop_ang_vel;     /* 1: x_init[10:13]=0 (comma-initialiser bug at
                               QuatMpc.cpp:242-245); 0: use ang_vel_body.  The default (1) is the
                               reference's behaviour; a closed loop around an ideal plant needs 0
                               beyond a few seconds                */
  int32_t model;            /* qmpc_model: which controller's problem the handle
                               solves (0 = QuatMpc, 1 = ConvexMpc)              */
} qmpc_params;

/* Fill *p with the Go1 values of gazebo_go1_quat_mpc.yaml and the solver
 * defaults for `mode`.  horizon: 10 or 20 in BASELINE.json. */
void qmpc_default_params(qmpc_params* p, int32_t horizon, int32_t mode);

/* ---- one MPC instance ----------------------------------------------------
 * Exactly the LeggedState fields grf_update reads, 48
 * doubles = 384 B, so one wavefront fetches one record with one coalesced
 * 8-byte-per-lane load. */
typedef struct qmpc_input {
  double quat[4];           /* fbk.torso_quat (w,x,y,z)       QuatMpc.cpp:236-239 */
  double rot[9];            /* fbk.torso_rot_mat, body->world :184-186,203,213   */
  double lin_vel_body[3];   /* R' * fbk.torso_lin_vel_world   :231               */
  double ang_vel_body[3];   /* fbk.torso_ang_vel_body (dropped when drop_ang_vel) */
  double foot_pos_body[12]; /* fbk.foot_pos_body, 3x4 col-major                  */
  double contacts[4];       /* ctrl.plan_contacts as 0.0 / 1.0 :118-125          */
  double pos_ref_body[3];   /* torso_pos_d_body_filtered      :156-158           */
  double vel_ref_body[3];   /* torso_lin_vel_d_body_filtered  :156-157,169       */
  double acc_ref_body[3];   /* 0 in QuatMpc; lets the accelerating reference of
                               TestAltroTrotQuatMpc.cpp:67-70 be expressed       */
  double quat_d[4];         /* ctrl.torso_quat_d AFTER the :128-137 update       */
} qmpc_input;

/* ---- one 8-contact-point instance (BASELINE config 5, synthetic) -----------
 * Same fields as qmpc_input with 8 contact points (two feet x 4 corner points):
 * 64 doubles = 512 B, one 8-byte-per-lane load of a whole wavefront. */
#define QMPC_NLEG8 8
#define QMPC_NU8 24
typedef struct qmpc_input8 {
  double quat[4];
  double rot[9];
  double lin_vel_body[3];
  double ang_vel_body[3];
  double foot_pos_body[24]; /* [3*point + axis]                                   */
  double contacts[8];
  double pos_ref_body[3];
  double vel_ref_body[3];
  double acc_ref_body[3];
  double quat_d[4];
} qmpc_input8;

/* ---- one ConvexMpc instance -------------------------
 * The LeggedState fields legged::ConvexMpc::grf_update reads
 * (legged_ctrl/src/mpc/ConvexMpc.cpp:81-198), again 48 doubles = 384 B.
 * State order of that controller: [roll pitch yaw, pos(3), ang_vel_world(3),
 * lin_vel_world(3)] (ConvexMpc.cpp:156-167); forces are WORLD-frame
 * (the caller rotates them: optimized_input = R' u, ConvexMpc.cpp:188-190). */
typedef struct qmpc_convex_input {
  double euler[3];            /* fbk.torso_euler                 ConvexMpc.cpp:156-158 */
  double pos_world[3];        /* fbk.torso_pos_world             :159-161             */
  double ang_vel_world[3];    /* fbk.torso_ang_vel_world         :162-164             */
  double lin_vel_world[3];    /* fbk.torso_lin_vel_world         :165-167             */
  double foot_pos_abs_com[12];/* fbk.foot_pos_abs_com, 3x4 col-major :115,118          */
  double contacts[4];         /* ctrl.plan_contacts as 0.0 / 1.0 :92,107-110          */
  double pos_d_world[3];      /* ctrl.torso_pos_d_world          :99-101              */
  double lin_vel_d_world[3];  /* ctrl.torso_lin_vel_d_world (x, y used; vz ref = 0) :105-107 */
  double yaw_rate_d;          /* ctrl.torso_ang_vel_d_body[2]    :98,104              */
  double reserved[13];        /* must be finite (0)                                    */
} qmpc_convex_input;

/* ---- per-instance result ------------------------------------------------- */
typedef struct qmpc_info {
  int32_t status;           /* qmpc_status                                     */
  int32_t iterations;       /* AL-iLQR iterations taken                        */
  double  cost;             /* final (un-augmented) objective                  */
  double  max_violation;    /* max(c,0) over all cone rows                     */
  double  last_step;        /* |dU|_inf of the final iteration [N]             */
  double  penalty;          /* final AL penalty                                */
} qmpc_info;

typedef struct qmpc_handle qmpc_handle;

/* ---- lifetime ------------------------------------------------------------ */
/* Creates a solver bound to HIP device `device` with capacity for `max_batch`
 * instances.  Fails with QMPC_NO_DEVICE when there is no GPU: there is NO CPU
 * fallback behind this library. */
qmpc_status qmpc_create(const qmpc_params* params, int32_t max_batch, int32_t device,
                        qmpc_handle** out);
qmpc_status qmpc_set_params(qmpc_handle* h, const qmpc_params* params);
void        qmpc_destroy(qmpc_handle* h);

/* ---- solve --------------------------------------------------------------- */
/* Synchronous, host buffers (replaces QuatMpc.cpp:217-265 for `batch`
 * independent LeggedStates).  forces_body: [batch][12]; info may be NULL;
 * traj_u ([batch][N][12]) and traj_x ([batch][N+1][13]) may be NULL (the first call that asks for a trajectory
 * allocates its device buffer, sized by max_batch; later calls reuse it).
 * batch == 1 keeps the blocking semantics of the reference's mpc_thread
 * (Main.cpp:106-108). */
qmpc_status qmpc_solve(qmpc_handle* h, int32_t batch, const qmpc_input* in,
                       double* forces_body, qmpc_info* info);
qmpc_status qmpc_solve_traj(qmpc_handle* h, int32_t batch, const qmpc_input* in,
                            double* forces_body, qmpc_info* info,
                            double* traj_u, double* traj_x);

/* Warm-started solve (QuatMpc handle, converged mode): every instance starts from u_init [batch][N][12] -- the caller's
 * previous solution of the same robot, e.g. the traj_u of last tick's call; it is shifted by one knot inside, swing legs
 * are pinned to 0 and a leg that has just landed starts from u_ref -- instead of u_ref (QuatMpc.cpp:253).  u_init NULL =
 * a cold solve.  traj_u [batch][N][12] (may be NULL; may be the same buffer as u_init) receives the new solution.  The
 * KKT point is the one qmpc_solve finds; with params.ipm_mu0 lowered to 1e-6 it takes about half the iterations for a
 * robot in its gait.  Host buffers / device buffers (stream-ordered). */
qmpc_status qmpc_solve_warm(qmpc_handle* h, int32_t batch, const qmpc_input* in, const double* u_init,
                            double* forces_body, qmpc_info* info, double* traj_u);
qmpc_status qmpc_solve_warm_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in, const double* d_u_init,
                                   double* d_forces_body, qmpc_info* d_info, double* d_traj_u, void* stream);

/* Stream-ordered, DEVICE buffers (inputs already resident in HBM).  `stream`
 * is a hipStream_t passed as void* (NULL = the handle's own stream).  Nothing
 * is synchronised; pair with qmpc_wait or your own stream sync.
 *
 * ONE launch in flight per HANDLE (not per stream): the handle owns mutable device state -- the gains workspace of the
 * mid-size kernels, the lane kernel's workspace / sort scratch, the hand-off list -- so a second qmpc_solve*_device on
 * the same handle must be stream-ordered after the first (same stream, or an event).  Independent batches in flight
 * take one handle each (bench.py: two_in_flight).
 *
 * Which kernel runs is chosen from the batch size (converged mode; QuatMpc N <= 12: everything in LDS up to 1024
 * instances, gains in a workspace up to 14335, from 14336 on one LANE per instance -- a lane PAIR while the batch fills only
 * half of every wavefront -- with the stragglers handed back to the wave kernel; N = 13 .. 22: the lane kernel from 14848;
 * warm-started launches: 18432 / 20480; the thresholds of the other models are in qmpc_hip.hip, and
 * qmpc_query(QMPC_QUERY_KERNEL_FOR_BATCH) answers for a given handle).  The kernel families solve the same
 * problem to the same KKT point but round differently: forces agree to ~1e-10 N across a threshold (tested to 1e-7 N),
 * bit for bit within a family and for a shard of a batch against the whole batch.  Their device buffers are allocated on
 * the first call that needs them, sized by max_batch, and held until qmpc_destroy: the lane kernel's workspace (<= 1024
 * wavefronts x 0.84 MB at N=10: 0.86 GB) and the state records of the straggler hand-off (8 + 84 N doubles per instance
 * of max_batch: 445 MB at 65536 x N=10) -- create the handle with the max_batch you mean to use. */
qmpc_status qmpc_solve_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in,
                              double* d_forces_body, qmpc_info* d_info, void* stream);
qmpc_status qmpc_wait(qmpc_handle* h);

/* Host buffers, NOT blocking: H2D copy, kernel and D2H copies are queued on the handle's stream and the call
 * returns; qmpc_wait(h) completes them.  `in`, `forces_body` and `info` must stay valid until then, and `in` must not
 * be modified before qmpc_wait when it is pinned (see below).  Lets the caller of the controller thread
 * (Main.cpp:103-118) do other work during the solve. */
qmpc_status qmpc_solve_async(qmpc_handle* h, int32_t batch, const qmpc_input* in,
                             double* forces_body, qmpc_info* info);

/* How the host-buffer calls (qmpc_solve, qmpc_solve_traj, qmpc_solve_async, qmpc_convex_solve*, qmpc_solve8*) move their
 * data -- SURVEY.md 8d's metric is exactly this call: records in host memory -> forces in host memory.
 *   - Batches that take a wave-per-instance kernel (every batch below the lane kernel's threshold: 14335 instances for QuatMpc at N <= 12; qmpc_query(QMPC_QUERY_KERNEL_FOR_BATCH) answers for a handle) run ZERO-COPY: every wavefront reads
 *     its 384-byte record from, and writes its forces / status record to, host memory the device can address.  Buffers
 *     from qmpc_host_alloc (or hipHostMalloc / hipHostRegister) are used in place; pageable buffers go through pinned
 *     staging the handle owns (one memcpy in, one out).  One launch, one synchronisation; results are bit-identical to
 *     qmpc_solve_device.  QMPC_ZERO_COPY=0 restores explicit copies.
 *   - Lane-kernel batches (which sort and re-read their records) use hipMemcpyAsync on the handle's stream; with pinned
 *     buffers those copies are true DMA. */
void*       qmpc_host_alloc(size_t bytes);      /* pinned, device-addressable host memory (NULL on failure) */
void        qmpc_host_free(void* p);

/* Allocate NOW whatever a solve (or closed loop) of up to `batch` instances on this handle needs later: the lane kernel's
 * workspace (<= 0.86 GB at N=10), the state records of the straggler hand-off (8 + 84 N doubles per instance of max_batch),
 * the pinned staging of the host-buffer calls.  After it returns no solve of up to `batch` instances allocates -- e.g.
 * inside the caller's own stream capture -- and qmpc_query tells whether the hand-off is available.  Optional: without it
 * the same buffers are allocated by the first call that needs them. */
qmpc_status qmpc_prepare(qmpc_handle* h, int32_t batch);

/* Handle state the results can depend on, and which kernel family a batch size selects. */
enum qmpc_query_what {
  QMPC_QUERY_HANDOFF_ACTIVE       = 1,  /* 1: lane-kernel batches hand their stragglers to the wave kernel (results: the
                                           hand-off's rounding family); 0: pure lane kernel (switched off, another model / mode,
                                           or the records could not be allocated -- ~1e-10 N apart, not bit-identical) */
  QMPC_QUERY_HANDOFF_ALLOC_FAILED = 2,  /* 1: the records' allocation failed on this handle (also reported on stderr) */
  QMPC_QUERY_KERNEL_FOR_BATCH     = 3,  /* arg = batch: the qmpc_kernel_family a plain solve of that size launches.
                                           It answers for a call with status records (info != NULL): without them a
                                           lane-kernel batch runs the pure lane kernel, never the hand-off */
  QMPC_QUERY_LAST_KERNEL          = 4,  /* family of the most recent solve launch */
  QMPC_QUERY_LANE_CAP             = 5,  /* arg = 1 plain solve / 2 cold closed loop / 3 warm closed loop: iteration cap of the
                                           capped lane launch (0: no hand-off) */
  QMPC_QUERY_DEVICE_BYTES         = 6,  /* device memory the handle holds right now */
  QMPC_QUERY_ZERO_COPY            = 7,  /* 1: host-buffer calls of wave-kernel batches run zero-copy */
  QMPC_QUERY_KERNEL_FOR_INSTANCES = 8,  /* arg = batch: the qmpc_kernel_family qmpc_solve_instances* launches for that size
                                           (QMPC_KERNEL_NONE: the handle refuses the call) */
  QMPC_QUERY_LOOP_INSTANCES_PLAN  = 9,  /* arg = batch (bits 0-31) | 1 << 32 with controller records | 1 << 33 with
                                           lp->warm_start: the launch qmpc_loop_run_instances* takes, 16 * form + family --
                                           form 1 the persistent kernel, 2 the per-tick sequence; family the
                                           qmpc_kernel_family of its solve.  0: the call is refused.  Bits 32 and 33 together
                                           answer under the handle's qmpc_set_loop_warm_records setting (default: refused;
                                           a ConvexMpc handle: under qmpc_set_convex_warm_records) */
  QMPC_QUERY_INSTANCES_POLICY     = 10, /* the handle's policy for qmpc_solve_instances*, a qmpc_instances_policy value */
  QMPC_QUERY_LOOP_WARM_RECORDS    = 11, /* 1: the closed loops with controller records accept lp->warm_start on this handle
                                           (qmpc_set_loop_warm_records); 0 (default): they refuse it */
  QMPC_QUERY_KERNEL_FOR_CONVEX_INSTANCES = 12, /* arg = batch: the qmpc_kernel_family qmpc_convex_solve_instances* launches
                                           for that size (QMPC_KERNEL_NONE, on a QuatMpc or 8-point handle too: the call is
                                           refused).  QMPC_QUERY_KERNEL_FOR_INSTANCES keeps answering NONE on a ConvexMpc handle */
  QMPC_QUERY_CONVEX_RECORDS       = 13, /* 1: the closed loops with per-robot records accept this ConvexMpc handle
                                           (qmpc_set_convex_records); 0 (default): they refuse it */
  QMPC_QUERY_CONVEX_LANE_RECORDS  = 14, /* 1: ConvexMpc's calls with per-instance records may take the lane kernel with per-lane
                                           parameters under QMPC_INSTANCES_AUTO (qmpc_set_convex_lane_records); 0 (default) */
  QMPC_QUERY_CONVEX_WARM_RECORDS  = 15, /* 1: the closed loops with controller records accept lp->warm_start on this ConvexMpc
                                           handle (qmpc_set_convex_warm_records, with qmpc_set_convex_records); 0 (default) */
  QMPC_QUERY_KERNEL_FOR_SCHEDULE  = 16  /* arg = batch: the qmpc_kernel_family qmpc_solve_schedule* launches for that size
                                           (QMPC_KERNEL_NONE: the handle refuses the call); the same under either
                                           qmpc_instances_policy */
};
enum qmpc_kernel_family {
  QMPC_KERNEL_NONE         = 0,
  QMPC_KERNEL_WFORM_LDS    = 1,   /* wave per instance, wrench form, everything in LDS */
  QMPC_KERNEL_WFORM_WS     = 2,   /* ... gains in the workspace */
  QMPC_KERNEL_DENSE_LDS    = 3,   /* wave per instance, dense 12x12 stage algebra (round-1 family), everything in LDS */
  QMPC_KERNEL_DENSE_WS     = 4,   /* ... gains (and slack arrays) in the workspace */
  QMPC_KERNEL_LANE         = 5,   /* lane per instance */
  QMPC_KERNEL_LANE_HANDOFF = 6    /* lane per instance to an iteration cap, stragglers continued by the wave kernel */
};
qmpc_status qmpc_query(qmpc_handle* h, int32_t what, int64_t arg, int64_t* value);

/* ---- per-instance robot and cost parameters (QuatMpc handle, converged mode) ----------------------------------------
 * One launch solves `batch` instances, each with its own robot and tuning: instance i is solved with the handle's
 * qmpc_params except for the seven fields of iparams[i] below (the handle's own values of those fields are ignored in
 * this call).  Horizon, knot spacing, mode, drop_ang_vel, tolerances and interior-point settings stay per handle, and so
 * do the reference's fixed trunk mass and CoM offset in the gravity torque.  Use cases: Monte-Carlo robustness sweeps
 * over payload, inertia and friction, fleets of differently loaded robots, sweeps over the cost weights.
 *
 * Per instance, a record with a non-finite field, mass <= 0, a singular inertia, an r_weight <= 0, a negative q_weight
 * or w, mu <= 0 or fz_max <= 0 gives that instance QMPC_BAD_PARAMS: zero forces, zero trajectory rows, 0 iterations.
 * The other instances are unaffected.  Call-level: QMPC_UNSUPPORTED for a ConvexMpc or 8-point handle, a reference-mode
 * handle, or a handle whose knobs leave no wrench-form kernel for the batch (QMPC_WFORM=0); QMPC_BATCH_TOO_LARGE above
 * max_batch; QMPC_BAD_ARGUMENT for null pointers.
 *
 * Kernel: the wave-per-instance wrench-form kernel a plain solve of the same size takes (everything in LDS, or the
 * workspace form), with its parameters read per workgroup; where the plain solve takes that kernel too, results are
 * bit-identical to qmpc_solve on a handle carrying the same values.  By default (QMPC_INSTANCES_WAVE) that holds at every
 * size: batches at and above the lane kernel's switch-over (14336 at N <= 12) stay on the wave workspace form (3.6 M
 * solves/s at N=10), and agree with the plain solve there to ~1e-10 N (another rounding family).
 *
 * The lane-per-instance form is chosen per handle: qmpc_set_instances_policy(h, QMPC_INSTANCES_AUTO).  From the measured
 * switch-over on (16384 instances at every horizon; the knob QMPC_LANE_INST_MIN overrides it) the call then runs
 * qmpc_lane_inst_kernel -- the plain lane kernel's passes with the seven record fields read per LANE from a parameter block
 * laid out like the lane workspace -- to the plain solve's iteration cap, and the per-instance list kernel continues the
 * stragglers (QMPC_KERNEL_LANE_HANDOFF; QMPC_KERNEL_LANE without status records or hand-off).  Below the switch-over AUTO
 * is the wave form above.  AUTO results belong to the lane / hand-off rounding family: ~1e-10 N from the wave family's, and
 * bit-identical to qmpc_solve's lane / hand-off results on a handle carrying the same values (forces, info, trajectories;
 * DESIGN.md section 3k).  Measured at N=10, random records: 6.2 M solves/s at 32768 and 7.2 M at 65536 instances, where the
 * wave form does 3.8 M and the plain solve 7.0 / 8.8 M.  Memory: the lane workspace and the
 * hand-off records of plain solves (qmpc_prepare) plus 312 B per resident lane of parameter rows; under AUTO
 * qmpc_prepare_instances and qmpc_prepare allocate them, under WAVE they allocate what they always did.  A handle that
 * refuses the call under WAVE refuses it under AUTO.
 *
 * Not covered: the reference mode, the 8-point model, warm starts.  ConvexMpc's problem has entry points of its own with
 * the same records, qmpc_convex_solve_instances* below.  The closed loop has its own entry points
 * with these records, qmpc_loop_run_instances* below; with controller records it keeps the wave form under either policy.
 *
 * The handle's per-instance buffers (the records and one expanded parameter block per instance, about 760 B x max_batch)
 * are allocated on first use, or now by qmpc_prepare_instances (e.g. before a stream capture). */
typedef struct qmpc_instance_params {   /* 38 doubles, 304 B */
  double mass;
  double inertia[9];        /* row-major, as qmpc_params.inertia */
  double mu;
  double fz_max;
  double q_weights[13];
  double r_weights[12];
  double w;
} qmpc_instance_params;

/* the seven fields of *p, as a record (e.g. to broadcast a handle's robot and edit one field per instance) */
void        qmpc_instance_params_from(const qmpc_params* p, qmpc_instance_params* out);
int32_t     qmpc_sizeof_instance_params(void);
/* Synchronous, host buffers: in [batch], iparams [batch], forces_body [batch][12]; info, traj_u ([batch][N][12]) and
 * traj_x ([batch][N+1][13]) may be NULL.  Copies explicitly on the handle's stream. */
qmpc_status qmpc_solve_instances(qmpc_handle* h, int32_t batch, const qmpc_input* in,
                                 const qmpc_instance_params* iparams, double* forces_body, qmpc_info* info,
                                 double* traj_u, double* traj_x);
/* Device buffers, stream-ordered (NULL stream = the handle's), nothing synchronised; d_info may be NULL.  Same rule as
 * qmpc_solve_device: one launch in flight per handle. */
qmpc_status qmpc_solve_instances_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in,
                                        const qmpc_instance_params* d_iparams, double* d_forces_body,
                                        qmpc_info* d_info, void* stream);
/* allocate the per-instance buffers now (qmpc_prepare does not); under QMPC_INSTANCES_AUTO also the lane kernel's */
qmpc_status qmpc_prepare_instances(qmpc_handle* h);
/* Which kernel family the calls with per-instance controller records may take on this handle -- qmpc_solve_instances* and the
 * per-tick solves of qmpc_loop_run_instances* / qmpc_loop_run_outcomes* with ctrl; holds until it is changed.
 * QMPC_BAD_ARGUMENT for a null handle or an unknown value.  qmpc_query(QMPC_QUERY_KERNEL_FOR_INSTANCES /
 * QMPC_QUERY_LOOP_INSTANCES_PLAN / QMPC_QUERY_LAST_KERNEL) answer under the current policy, and qmpc_prepare allocates for it. */
typedef enum qmpc_instances_policy {
  QMPC_INSTANCES_WAVE = 0,   /* default: the wave wrench-form kernels at every size */
  QMPC_INSTANCES_AUTO = 1    /* lane per instance (with the straggler hand-off) from the switch-over on: 16384 instances in
                                qmpc_solve_instances* and in the closed loops' ticks with controller records */
} qmpc_instances_policy;
qmpc_status qmpc_set_instances_policy(qmpc_handle* h, int32_t policy);

/* ---- a contact schedule over the horizon (QuatMpc handle, converged mode, four contact points) ------------------------------
 * qmpc_input::contacts pins a leg to stance or swing at all N knots (QuatMpc.cpp:118-125 does the same).  These calls take
 * the stance set PER KNOT: schedule[b][k], k = 0 ... N-1, one byte per knot, bit l set where leg l stands during knot k
 * (qmpc_gait_predict below writes such rows from a robot's gait state).  The problem of instance b:
 *   - a leg in the air at a knot carries exactly zero force there and is no variable there; traj_u[k][3l ..] is +0.0
 *   - the cone rows of a (knot, leg) exist only where the bit is set
 *   - the input reference is the knot's: u_ref_k[3l+2] = c_kl mass 9.81 / nc_k, nc_k the number of legs standing at knot k
 *   - dynamics, state cost, attitude cost, references and foot_pos_body (ONE position per leg for the whole horizon) are those
 *     of qmpc_solve.  For a leg that is in the air now and lands inside the horizon the caller sets foot_pos_body[l] to the
 *     touchdown point: the leg's foot_target_world, taken to the body frame like the other feet.  No knot-0 arithmetic reads
 *     the position of a leg that is in the air at knot 0.
 *   - qmpc_input::contacts is NOT read.  Knot 0 of the schedule decides which legs get a force: forces_body is knot 0 of the
 *     solution.
 * A schedule that repeats the record's contacts at every knot gives qmpc_solve_instances*' wave-kernel results bit for bit
 * (forces, info, trajectories).
 *
 * iparams: per-instance robot and cost records as in qmpc_solve_instances, or NULL: the handle's own values for every
 * instance.  Per instance: a knot without a stance leg gives QMPC_NO_CONTACT (flight phases are not covered), a byte above 15
 * QMPC_BAD_PARAMS, an invalid record QMPC_BAD_PARAMS; each with zero forces, zero trajectory rows and 0 iterations, the other
 * instances unaffected.  Call level: QMPC_UNSUPPORTED for a ConvexMpc or 8-point handle, a reference-mode handle, or a handle
 * whose knobs leave no wrench-form kernel (QMPC_WFORM=0); QMPC_BATCH_TOO_LARGE above max_batch; QMPC_BAD_ARGUMENT for a null
 * in, schedule or forces_body.
 *
 * Kernel: qmpc_solve_w_sched_kernel, the wave-per-instance wrench-form kernel of qmpc_solve_instances with the stance set
 * asked per knot -- the variant that call takes for the size under QMPC_INSTANCES_WAVE, under either policy (the lane kernel
 * has no schedule form).  qmpc_query(QMPC_QUERY_KERNEL_FOR_SCHEDULE) names the family for a batch size,
 * QMPC_QUERY_LAST_KERNEL the one the last call took.  Buffers: those of qmpc_prepare_instances, and for the host-buffer call
 * N bytes per instance of schedule staging, allocated on first use and counted in QMPC_QUERY_DEVICE_BYTES.
 * Not covered: warm starts, the closed loops, the lane kernel, ConvexMpc, the 8-point model, the reference mode, a second
 * foothold per leg inside one horizon. */
/* Synchronous, host buffers: in [batch], iparams [batch] or NULL, schedule [batch][N], forces_body [batch][12]; info, traj_u
 * ([batch][N][12]) and traj_x ([batch][N+1][13]) may be NULL. */
qmpc_status qmpc_solve_schedule(qmpc_handle* h, int32_t batch, const qmpc_input* in,
                                const qmpc_instance_params* iparams, const uint8_t* schedule, double* forces_body,
                                qmpc_info* info, double* traj_u, double* traj_x);
/* Device buffers, stream-ordered (NULL stream = the handle's), nothing synchronised; d_iparams, d_info, d_traj_u and d_traj_x
 * may be NULL.  One launch in flight per handle. */
qmpc_status qmpc_solve_schedule_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in,
                                       const qmpc_instance_params* d_iparams, const uint8_t* d_schedule,
                                       double* d_forces_body, qmpc_info* d_info, double* d_traj_u, double* d_traj_x,
                                       void* stream);

/* ---- per-instance robot and cost parameters for ConvexMpc's problem (ConvexMpc handle, converged mode) ------------------
 * qmpc_solve_instances* for the sibling controller: qmpc_convex_input records, world-frame forces, and the same 304-byte
 * qmpc_instance_params -- e.g. one fleet with its payload, inertia and friction spread, solved under both controllers.
 * ConvexMpc reads mass, inertia, mu, fz_max, q_weights[0..11] (its state has 12 entries) and r_weights from a record;
 * q_weights[12] and w are validated like the other fields and otherwise unused.  The handle's own values of those fields
 * are ignored in this call.  A record is invalid by the rule above (QMPC_BAD_PARAMS for that instance: zero forces, zero
 * trajectory rows, 0 iterations; its neighbours are unaffected).
 *
 * Kernel: qmpc_solve_cw_inst_kernel, the wrench-form ConvexMpc kernel with its parameters read per workgroup, on the
 * variant (everything in LDS / gains / gains and slack arrays in the workspace) a plain qmpc_convex_solve of the size takes
 * on the wrench form; results are then bit-identical to qmpc_convex_solve on a handle carrying the same values.  Where the
 * plain solve takes the round-1 kernel or the lane kernel (there is no per-instance form of either for this problem) the
 * call stays on a wrench-form variant and agrees with the plain solve to the rounding between ConvexMpc's kernel families
 * (status words equal, forces within 1e-7 N).  qmpc_query(QMPC_QUERY_KERNEL_FOR_CONVEX_INSTANCES) names the family for a
 * batch size, QMPC_QUERY_LAST_KERNEL the one the last call took.  By default qmpc_set_instances_policy does not change this
 * call; the lane-per-instance form with per-lane parameters is a setting of the handle, qmpc_set_convex_lane_records below.
 *
 * Call-level: QMPC_UNSUPPORTED on a QuatMpc or 8-point handle, a reference-mode handle, or a handle whose knobs leave no
 * wrench-form kernel (QMPC_WFORM=0); QMPC_BATCH_TOO_LARGE above max_batch; QMPC_BAD_ARGUMENT for null pointers.  The
 * buffers are those of qmpc_prepare_instances (which a ConvexMpc handle in the converged mode accepts too).
 *
 * Host buffers: in [batch], iparams [batch], forces_world [batch][12]; info, traj_u ([batch][N][12]) and traj_x
 * ([batch][N+1][12]) may be NULL.  Synchronous. */
qmpc_status qmpc_convex_solve_instances(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in,
                                        const qmpc_instance_params* iparams, double* forces_world, qmpc_info* info,
                                        double* traj_u, double* traj_x);
/* Device buffers, stream-ordered (NULL stream = the handle's), nothing synchronised; d_info may be NULL. */
qmpc_status qmpc_convex_solve_instances_device(qmpc_handle* h, int32_t batch, const qmpc_convex_input* d_in,
                                               const qmpc_instance_params* d_iparams, double* d_forces_world,
                                               qmpc_info* d_info, void* stream);

/* Multi-GPU: the single collective of the path.  All-gathers `count` doubles per rank (e.g. the
 * [B/G][12] force block, or forces + qmpc_info records laid out in one buffer) from every rank's `d_local` into
 * `d_all` ([ranks * count], rank order) with RCCL's ncclAllGather on `stream` (NULL = the handle's stream),
 * stream-ordered after the solve that produced `d_local`.  `nccl_comm` is the caller's ncclComm_t (one per GPU /
 * process, created by the host program).  RCCL is looked up at run time; QMPC_UNSUPPORTED when it is absent. */
qmpc_status qmpc_gather(qmpc_handle* h, void* nccl_comm, const double* d_local, int64_t count,
                        double* d_all, void* stream);

/* Time (ms, HIP events on the launch stream) of the most recent
 * qmpc_solve_device / qmpc_solve kernel, after it completed. */
qmpc_status qmpc_last_kernel_ms(qmpc_handle* h, float* ms);

/* Batched linearisation only: for every instance and knot
 * k<N, roll out x from the reference's initial guess U=u_ref and return the
 * error-state Jacobians  Abar [batch][N][12][12], Bbar [batch][N][12][12]
 * (row-major) and the rollout X [batch][N+1][13].  Host buffers. */
qmpc_status qmpc_linearize(qmpc_handle* h, int32_t batch, const qmpc_input* in,
                           double* Abar, double* Bbar, double* X);

/* ---- ConvexMpc entry points (handle created with params.model = QMPC_MODEL_CONVEX)
 * Replace ConvexMpc.cpp:84-186 (ALTRO set-up, Solve(), GetInput(0)).
 * forces_world: [batch][12]; traj_u [batch][N][12], traj_x [batch][N+1][12] may be NULL.
 * Calling a quaternion entry point on a convex handle (or vice versa) returns
 * QMPC_BAD_ARGUMENT. */
void        qmpc_default_convex_params(qmpc_params* p, int32_t horizon, int32_t mode);
qmpc_status qmpc_convex_solve(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in,
                              double* forces_world, qmpc_info* info);
qmpc_status qmpc_convex_solve_traj(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in,
                                   double* forces_world, qmpc_info* info,
                                   double* traj_u, double* traj_x);
qmpc_status qmpc_convex_solve_device(qmpc_handle* h, int32_t batch, const qmpc_convex_input* d_in,
                                     double* d_forces_world, qmpc_info* d_info, void* stream);
/* Discrete Jacobians A [batch][N][12][12], B [batch][N][12][12] (row-major, as the
 * reference's midpoint_jacobian of ct_srb_jacobian produces them, AltroUtils.cpp:78-110,
 * 297-359) along the rollout X [batch][N+1][12] of U = u_ref.  Host buffers. */
qmpc_status qmpc_convex_linearize(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in,
                                  double* A, double* B, double* X);

/* ---- 8-contact-point entry points (handle created with params.model = QMPC_MODEL_QUAT8)
 * forces_body: [batch][24]; traj_u [batch][N][24], traj_x [batch][N+1][13] may be NULL.
 * r_weights[j % 12] is used for input j.  The defaults are a synthetic 30 kg biped
 * (stated in DESIGN.md); nothing in the reference pins them. */
void        qmpc_default_biped8_params(qmpc_params* p, int32_t horizon, int32_t mode);
qmpc_status qmpc_solve8(qmpc_handle* h, int32_t batch, const qmpc_input8* in,
                        double* forces_body, qmpc_info* info);
qmpc_status qmpc_solve8_traj(qmpc_handle* h, int32_t batch, const qmpc_input8* in,
                             double* forces_body, qmpc_info* info, double* traj_u, double* traj_x);
qmpc_status qmpc_solve8_device(qmpc_handle* h, int32_t batch, const qmpc_input8* d_in,
                               double* d_forces_body, qmpc_info* d_info, void* stream);

/* ---- force -> joint-torque consumer --------------------
 * The step right after the path: BaseInterface::tau_ctrl_update
 * (legged_ctrl/src/interfaces/BaseInterface.cpp:343-408) maps the body-frame foot
 * forces to joint torques, tau_leg = -J_leg(q)' f_leg (:368,401), with the leg
 * Jacobian of A1Kinematics::jac (legged_ctrl/src/utils/A1Kinematics.cpp:15-19,
 * evaluated in fbk.jac_foot at BaseInterface.cpp:209-212).  Batched here so that
 * Monte-Carlo sweeps get joint torques without leaving the GPU.
 * Leg geometry = the reference's rho_fix / rho_opt vectors (BaseInterface.cpp:10-34). */
typedef struct qmpc_leg_geometry {
  double rho_fix[4][5];     /* per leg: offset_x, offset_y, motor_offset, upper, lower length */
  double rho_opt[4][3];     /* per leg: contact-point offsets (0 in the reference)           */
} qmpc_leg_geometry;
void qmpc_default_go1_geometry(qmpc_leg_geometry* g);   /* BaseInterface.cpp:12-26, LeggedParams.h:14-15 */

/* Foot position in the body frame and leg Jacobian for every instance and leg
 * (A1Kinematics::fk / ::jac).  joint_pos [batch][12] (leg-major: hip, thigh, calf);
 * foot_pos_body [batch][12] (3x4 col-major, [3*leg+axis]); jac [batch][4][9], each
 * 3x3 COLUMN-major like Eigen's Matrix3d::data().  Either output may be NULL.  Host buffers. */
qmpc_status qmpc_leg_kinematics(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                const double* joint_pos, double* foot_pos_body, double* jac);
/* tau [batch][12] = -J' f per leg; legs with contacts == 0 get zero torque when
 * `walking` != 0 (movement_mode > 0, BaseInterface.cpp:366-370); with walking == 0
 * every leg is mapped (:401).  contacts [batch][4] may be NULL (= all stance).  Host buffers. */
qmpc_status qmpc_torque_map(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                            const double* joint_pos, const double* forces_body,
                            const double* contacts, int32_t walking, double* tau);
/* Same with DEVICE buffers, stream-ordered (NULL = the handle's stream), e.g. straight
 * after qmpc_solve_device on the forces it produced. */
qmpc_status qmpc_torque_map_device(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                   const double* d_joint_pos, const double* d_forces_body,
                                   const double* d_contacts, int32_t walking, double* d_tau,
                                   void* stream);

/* ---- the whole low-level command of a tick (completed) -----
 * BaseInterface::tau_ctrl_update (BaseInterface.cpp:343-408) turns the outputs of grf_update into what the
 * 1 kHz joint loop sends to the motors: per leg
 *   walking (movement_mode > 0):
 *     joint_ang_tgt = inv_kin(R'(optimized_state[6+3i] - torso_pos_world), joint_pos)     (:349-355; NaN -> joint_pos)
 *     joint_vel_tgt = J^-1 R'(optimized_input[12+3i] - torso_lin_vel_world)               (:358-364; NaN -> joint_vel)
 *     joint_tau_tgt = plan_contacts ? -J' optimized_input[3i] : 0                         (:367-371)
 *   standing: joint_tau_tgt = -J' f, targets = the measured joint_pos / joint_vel          (:400-403)
 * with J = A1Kinematics::jac(joint_pos) (BaseInterface.cpp:209-212) and A1Kinematics::inv_kin
 * (A1Kinematics.cpp:335-459: closed-form, single-precision atan2 approximation :291-312, the hip-angle branch
 * nearest to the current angle). */
typedef struct qmpc_joint_feedback {
  double joint_pos[12], joint_vel[12];                     /* fbk.joint_pos / joint_vel, leg-major (hip, thigh, calf)  */
  double torso_pos_world[3], torso_quat[4] /* w,x,y,z */, torso_lin_vel_world[3];
  double foot_pos_target_world[12];                        /* ctrl.optimized_state.segment<12>(6),  QuatMpc.cpp:270    */
  double foot_vel_target_world[12];                        /* ctrl.optimized_input.segment<12>(12), QuatMpc.cpp:271    */
  double forces_body[12];                                  /* ctrl.optimized_input.segment<12>(0),  QuatMpc.cpp:267    */
  double plan_contacts[4];                                 /* ctrl.plan_contacts (0 / 1)                               */
  double movement_mode;
} qmpc_joint_feedback;                                     /* 75 doubles */
typedef struct qmpc_joint_command {
  double joint_ang_tgt[12], joint_vel_tgt[12], joint_tau_tgt[12];
} qmpc_joint_command;                                      /* 36 doubles */
/* A1Kinematics::inv_kin for every instance and leg: foot_pos_body [batch][12], cur_joint_pos [batch][12] (branch
 * selection), joint_pos [batch][12] out (NaN where the foot is out of reach, as in the reference).  Host buffers. */
qmpc_status qmpc_leg_inverse_kinematics(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                        const double* foot_pos_body, const double* cur_joint_pos, double* joint_pos);
/* tau_ctrl_update for `batch` robots.  Host buffers / device buffers (stream-ordered, NULL = the handle's stream). */
qmpc_status qmpc_joint_commands(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                const qmpc_joint_feedback* fb, qmpc_joint_command* cmd);
qmpc_status qmpc_joint_commands_device(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                       const qmpc_joint_feedback* d_fb, qmpc_joint_command* d_cmd, void* stream);

/* ---- device-resident closed loop -----------------------
 * The step BEFORE the path, the path and a plant chained on the GPU, state kept in HBM, one tick =
 *   feedback  (R, R_z, foot_pos_body, contact flags from the plant state)
 *   Raibert foothold targets              BaseInterface.cpp:266-288
 *   goal_update                            QuatMpc.cpp:68-107  (six 100-sample moving averages, MovingWindowFilter.hpp)
 *   foot_update: gait FSM + swing quintic  QuatMpc.cpp:278-305, LeggedContactFSM.cpp:33-86,208-246, Utils.cpp:236-293
 *   record packing (torso_quat_d update)   QuatMpc.cpp:112-176,231-246
 *   qmpc_solve_device                      QuatMpc.cpp:217-265
 *   outputs                                QuatMpc.cpp:263-273
 *   plant: single rigid body under the forces, explicit midpoint, dt = 5 ms (this repository's; the reference
 *          closes its loop through Gazebo / the robot); swing feet track the FSM target, stance feet stay.
 * The host classes (host/QuatMpcHip.h + host/ClosedLoopHost.h) run the same tick on the CPU and are the parity
 * reference, tick for tick.  Integers are stored as doubles so that the record is 820 doubles for every binding. */
#define QMPC_LOOP_WINDOW 100
typedef struct qmpc_loop_filter {      /* MovingWindowFilter.hpp:14-63 */
  double ring[QMPC_LOOP_WINDOW];
  double head, count, sum, correction;
} qmpc_loop_filter;
typedef struct qmpc_loop_leg {         /* LeggedContactFSM.h:60-108 */
  double gait_phase, state /* 0 swing, 1 stance */, pattern_index, prev_pattern_index, start_time, end_time,
         not_first_call;
  double swing_start[3], swing_end[3], swing_extend[3];
  double fsm_pos[3], fsm_vel[3], fsm_acc[3];   /* FSM_foot_{pos,vel,acc}_target_world */
  double terrain_height;
} qmpc_loop_leg;
typedef struct qmpc_loop_state {
  /* plant */
  double pos_world[3], quat[4], lin_vel_world[3], ang_vel_body[3], foot_pos_world[12];
  /* command: joy.{velx, vely, body_height, roll_rate, pitch_rate, yaw_rate}, ctrl.movement_mode */
  double joy[6], movement_mode;
  double sin_ang_vel, attitude_traj_count;   /* joy.sin_ang_vel (LeggedState.h:157): the reference's attitude-sweep test mode,
                                                torso_quat_d = euler_to_quat(pi/8 sin(2 pi k / 900) (1,1,1)), QuatMpc.cpp:138-146 */
  /* controller memory */
  double pos_d_world[3], pos_d_init, quat_d[4], lin_vel_d_rel[3];
  qmpc_loop_filter vel_filter[3], pos_filter[3];
  qmpc_loop_leg leg[4];
  /* outputs of the last tick */
  double contacts[4], gait_counter[4], forces_body[12], grf_world[12], foot_target_world[12];
  double status, iterations, tick;
} qmpc_loop_state;
typedef struct qmpc_loop_params {
  double gait_freq;                 /* param.gait_freq (yaml: 2.2)                      */
  double default_foot_pos_rel[12];  /* param.default_foot_pos_rel, [3*leg+axis]         */
  double dt;                        /* tick: the reference's hard-wired 5 ms (QuatMpc.cpp:97-98,132,294) */
  double contact_height;            /* plant: foot_contact_flag = foot z <= this [m]    */
  double warm_start;                /* 0 (default): every solve starts from u_ref like the reference (QuatMpc.cpp:253).
                                       != 0: from the second tick of a call on, the solve starts from the previous
                                       tick's solution shifted by one knot (swing legs 0, a leg that has just landed
                                       from u_ref); converged mode.  The persistent kernel keeps that solution in LDS,
                                       the per-tick form in the handle's trajectory buffer.  Same KKT points, about half the iterations when
                                       combined with a low params.ipm_mu0 (1e-6): DESIGN.md 3e */
} qmpc_loop_params;
void qmpc_default_loop_params(qmpc_loop_params* p);
/* Host-side initialiser (no GPU involved): robot standing at `height` over its default footholds, at rest,
 * yaw `yaw`; joy[6] and movement_mode as above. */
void qmpc_loop_state_init(qmpc_loop_state* s, const qmpc_loop_params* lp, const double joy[6], double movement_mode,
                          double height, double yaw);
/* `ticks` ticks for `batch` instances.  Host buffers in/out; trace_forces [ticks][batch][12] (body frame) and
 * trace_contacts [ticks][batch][4] may be NULL.  The handle is a QuatMpc handle (QMPC_MODEL_QUAT, either solver mode) or a
 * ConvexMpc handle (QMPC_MODEL_CONVEX, either solver mode): the latter runs ConvexMpc's tick -- its goal_update
 * (ConvexMpc.cpp:51-79; pos_d_world[0:2] hold joy.body_x / body_y, roll / pitch rate commands are ignored), its feedback
 * and record, R' u into the plant -- with host/ClosedLoopHost.h over ConvexMpcHipT as the parity reference.  The device
 * tick of ConvexMpc carries the controller period as the literal 5 ms (as the QuatMpc tick does upstream): a ConvexMpc
 * handle whose knot spacing params.h is not 5 ms is refused with QMPC_UNSUPPORTED. */
qmpc_status qmpc_loop_run(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                          int32_t ticks, double* trace_forces, double* trace_contacts);
/* The same with DEVICE buffers, stream-ordered (NULL = the handle's stream).  Up to 2048 robots (4096 with
 * lp->warm_start) the whole loop is ONE launch of a persistent kernel in which a wavefront owns a robot for all ticks
 * (both controllers, both solver modes); beyond, the per-tick kernel sequence is captured once into a hipGraph and
 * replayed `ticks` times.  The two forms give the same bits (QMPC_LOOP_FUSED=0 / 1 forces one).
 * For roll-outs longer than a few seconds set params.drop_ang_vel = 0 (see qmpc_params). */
qmpc_status qmpc_loop_run_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                 int32_t ticks, double* d_trace_forces, double* d_trace_contacts, void* stream);
int32_t qmpc_sizeof_loop_state(void);
/* Joint-level commands of the robots of a closed loop, from their states after a tick (device buffers): the plant has
 * massless legs, so the measured joint angles are inv_kin of the plant's foot positions; d_joint_pos [batch][12] is
 * in/out (in: the angles of the previous tick, which select the hip branch - initialise with
 * qmpc_loop_joint_init; out: this tick's), the joint velocities are J^-1 R'(foot velocity - torso velocity) with
 * swing feet moving at their FSM target velocity.  d_fb (may be NULL) receives the feedback records that were built,
 * d_cmd the commands: exactly qmpc_joint_commands_device on those records. */
qmpc_status qmpc_loop_joint_commands_device(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                            const qmpc_loop_state* d_states, double* d_joint_pos,
                                            qmpc_joint_feedback* d_fb, qmpc_joint_command* d_cmd, void* stream);
/* The same with HOST buffers (states as qmpc_loop_run leaves them; fb may be NULL). */
qmpc_status qmpc_loop_joint_commands(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                     const qmpc_loop_state* states, double* joint_pos, qmpc_joint_feedback* fb,
                                     qmpc_joint_command* cmd);
/* The closed loop down to the motors: qmpc_loop_run_device with the joint level closing every tick (inside the
 * persistent kernel, or as the fourth kernel of the captured per-tick graph).  d_joint_pos [batch][12] in/out as above;
 * d_cmd [batch] receives the commands of the LAST tick, d_trace_cmd [ticks][batch] those of every tick (either may be
 * NULL, not both). */
qmpc_status qmpc_loop_run_joint_device(qmpc_handle* h, const qmpc_loop_params* lp, const qmpc_leg_geometry* g,
                                       int32_t batch, qmpc_loop_state* d_states, double* d_joint_pos, int32_t ticks,
                                       qmpc_joint_command* d_cmd, qmpc_joint_command* d_trace_cmd, void* stream);

/* ---- closed loop with per-robot controller and plant (QuatMpc handle, converged mode) --------------------------------
 * One launch sequence runs `batch` robots, each with its own controller tuning and its own TRUE robot: the question of a
 * Monte-Carlo robustness sweep (does the robot stay up and track its command when the real robot differs from the one
 * its controller assumes?) and of fleets of differently loaded robots.  Everything else is the closed loop of
 * qmpc_loop_run_device: the same tick, the persistent kernel or the captured per-tick graph, the same traces.
 *
 *   ctrl[i]   robot i's controller: the handle's qmpc_params with the seven fields of ctrl[i] in place, exactly as in
 *             qmpc_solve_instances.  NULL: the handle's parameters for every robot.
 *   plant[i]  robot i's plant integrates with plant[i].mass and .inertia and adds the constant disturbance wrench
 *             (ext_force_world at the CoM in the world frame, ext_torque_body in the body frame).  NULL: each robot's
 *             plant is its controller's robot -- ctrl[i]'s mass and inertia, or the handle's where ctrl is NULL -- with no
 *             disturbance.  A disturbance component that is exactly zero adds no arithmetic: a record with zero
 *             disturbance integrates to the bits of the plain loop's plant with the same mass and inertia.
 *   both NULL exactly qmpc_loop_run_device.
 *
 * Invalid records: a controller record by the rule of qmpc_solve_instances; a plant record with a non-finite field,
 * mass <= 0 or a singular inertia.  The robot of an invalid record is FROZEN: its state record is left untouched except
 * status = QMPC_BAD_PARAMS and iterations = 0 (tick does not advance), its trace rows are zero.  Every other robot is
 * unaffected, bit for bit.
 *
 * Call level: QMPC_BAD_ARGUMENT for null pointers and for an 8-point handle (as qmpc_loop_run); QMPC_UNSUPPORTED, when
 * ctrl or plant is non-NULL, for a reference-mode handle and for a ConvexMpc handle that has not opted in
 * (qmpc_set_convex_records below; off by default); with ctrl non-NULL also for lp->warm_start != 0
 * unless the handle opted in (qmpc_set_loop_warm_records below; off by default) and for a handle whose knobs leave no
 * wrench-form kernel (QMPC_WFORM=0); QMPC_BATCH_TOO_LARGE above max_batch.  With
 * plant only, everything the plain loop supports works, the warm start included, and the per-tick form keeps the plain
 * loop's solve (lane kernel and hand-off included).  Joint commands are not part of these calls: run
 * qmpc_loop_joint_commands_device on the states afterwards.  Motor torque limits inside the loop: qmpc_loop_run_motors* below.
 *
 * Launch (qmpc_query QMPC_QUERY_LOOP_INSTANCES_PLAN): the persistent kernel up to the plain loop's threshold (2048
 * robots, 4096 warm) on the wrench-form variant the plain loop takes; beyond, the per-tick sequence, whose solve is the
 * per-instance wrench-form kernel (qmpc_solve_instances*) with ctrl, the plain loop's solve without.  The records are
 * expanded once per call.  Buffers: those of qmpc_prepare_instances (764 B x max_batch) and per-robot plant blocks
 * (264 B x max_batch), allocated on first use; a call with ticks = 0 allocates both and launches nothing (e.g. before
 * the caller's own stream capture).  The per-tick form captures its tick after every allocation.
 *
 * Under qmpc_set_instances_policy(h, QMPC_INSTANCES_AUTO) the per-tick solve with ctrl takes the lane kernel from the
 * switch-over on (the larger of qmpc_solve_instances*' and the cold-started loop's: 16384 robots; QMPC_LANE_INST_MIN and
 * QMPC_LANE_MIN move it): in every tick the stance sort -- ordered by the previous tick's iteration counts too, robots that
 * will not solve (invalid record, frozen, halted) in a class of their own at the end, where they fill whole wavefronts that
 * leave at once -- then qmpc_lane_inst_kernel to the loop's iteration cap and the per-instance list kernel on the stragglers
 * (QMPC_KERNEL_LANE_HANDOFF; QMPC_KERNEL_LANE without hand-off).  The results then belong to the lane / hand-off rounding
 * family: with uniform records the bytes of qmpc_loop_run_device at the same size, ~1e-10 N per solve from the wave
 * family's.  Below the switch-over, without ctrl and under the default policy nothing changes, bit for bit.  The lane
 * kernel's buffers (workspace, sort scratch, per-lane parameter rows, hand-off records) are allocated before the tick is
 * captured, by a call with ticks = 0 too, and by qmpc_prepare(h, batch) under AUTO when `batch` robots with ctrl take
 * this form; under the default policy no call allocates them.
 *
 * Warm start with controller records: qmpc_set_loop_warm_records(h, 1).  lp->warm_start != 0 is then accepted with ctrl by
 * qmpc_loop_run_instances*, qmpc_loop_run_outcomes* and qmpc_loop_run_pushes*, with the plain loop's rule: the first tick of a
 * call starts cold, every later solve of a robot starts from its previous solution shifted by one knot unless that solve
 * failed (a robot that was frozen or halted never solved).  Launch: the persistent kernel up to 4096 robots, as with plant
 * records only; beyond, the per-tick sequence whose later ticks run qmpc_solve_w_inst_warm_kernel on the variant of
 * qmpc_solve_instances* -- the solution travels through the handle's trajectory buffer -- and, under QMPC_INSTANCES_AUTO from
 * the larger of qmpc_solve_instances*' switch-over and the warm-started loop's on (18432 robots at N <= 12, 20480 at
 * N = 13 ... 22), the stance sort, qmpc_lane_inst_warm_kernel to the warm ticks' iteration cap (qmpc_query QMPC_QUERY_LANE_CAP,
 * arg 3) and the per-instance list kernel on the stragglers; the cold first tick of a call runs the lane kernel without cap and
 * hand-off, so QMPC_QUERY_LAST_KERNEL after a call of one tick says QMPC_KERNEL_LANE where the plan says LANE_HANDOFF.  With uniform records every form gives the bytes of
 * qmpc_loop_run_device with the same lp at the same size.  The buffers this adds (the trajectory buffer, 96 N bytes x
 * max_batch; the lane kernel's under AUTO) are allocated before the tick is captured, by a call with ticks = 0 too, and by
 * qmpc_prepare.  After such a call the device entry points may run inside a stream capture of the CALLER's (persistent form and
 * per-tick wave form; the ticks become nodes of the caller's graph, and the library begins no capture of its own inside it); a handle that never opts in plans, refuses, computes and allocates as before. */
typedef struct qmpc_plant_params {   /* 16 doubles, 128 B: the TRUE robot the plant integrates */
  double mass;
  double inertia[9];                 /* row-major, same convention as qmpc_params.inertia */
  double ext_force_world[3];         /* constant disturbance at the CoM, world frame [N] */
  double ext_torque_body[3];         /* constant disturbance torque, body frame [N m] */
} qmpc_plant_params;
/* mass and inertia of *p, zero disturbance */
void    qmpc_plant_params_from(const qmpc_params* p, qmpc_plant_params* out);
int32_t qmpc_sizeof_plant_params(void);
/* Host buffers: states [batch] in/out, ctrl / plant [batch] (either may be NULL), trace_forces [ticks][batch][12] and
 * trace_contacts [ticks][batch][4] may be NULL.  Synchronous. */
qmpc_status qmpc_loop_run_instances(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                    int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                    double* trace_forces, double* trace_contacts);
/* Device buffers, stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_instances_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                           qmpc_loop_state* d_states, int32_t ticks,
                                           const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                           double* d_trace_forces, double* d_trace_contacts, void* stream);
/* on = 1: the closed loops with controller records (the three pairs of entry points with ctrl) accept lp->warm_start on this
 * handle; 0 (default): they refuse it with QMPC_UNSUPPORTED.  Holds until it is changed.  QMPC_BAD_ARGUMENT for a null handle
 * or another value.  qmpc_query(QMPC_QUERY_LOOP_WARM_RECORDS) returns the setting, QMPC_QUERY_LOOP_INSTANCES_PLAN answers
 * under it. */
qmpc_status qmpc_set_loop_warm_records(qmpc_handle* h, int32_t on);

/* Opt in to the closed loops with per-robot records on a ConvexMpc handle: on = 1 (0, the default, restores the refusal).
 * qmpc_loop_run_instances*, qmpc_loop_run_outcomes* and qmpc_loop_run_pushes* then accept a ConvexMpc handle in the converged
 * mode -- with ctrl and / or plant, with outcome records and stop_when_down, with push windows -- with the semantics, buffers
 * and ticks = 0 behaviour they have on a QuatMpc handle: the same fleet, plants, pushes and outcome records under either
 * controller.  A controller record is read as by qmpc_convex_solve_instances*; the plant step is the one of the QuatMpc calls,
 * on the world-frame forces of ConvexMpc rotated into the body (optimized_input = R' u).  A handle that never opts in plans,
 * refuses, computes and allocates as before; the setting does nothing on a handle of another model.
 *
 * Launch (QMPC_QUERY_LOOP_INSTANCES_PLAN answers under the setting): the persistent kernel where the plain ConvexMpc loop of
 * the batch takes its own on a wrench-form variant (2048 robots, 4096 with lp->warm_start, or QMPC_LOOP_FUSED); otherwise per
 * tick -- the front kernel, qmpc_solve_cw_inst_kernel with ctrl or the plain ConvexMpc tick (its lane kernel included) without,
 * the post kernel.  With records equal to the handle's values both forms give the bytes of qmpc_loop_run* on the same handle
 * (states, force and contact traces) wherever that loop solves on the same wrench-form variant, and the two forms agree with
 * each other bit for bit on any records.  Under QMPC_INSTANCES_AUTO the ticks with ctrl stay on the wave kernels at every
 * size unless the handle also opted in to the lane form (qmpc_set_convex_lane_records below).
 *
 * Still QMPC_UNSUPPORTED with the setting on: the reference mode; ctrl together with lp->warm_start, whatever
 * qmpc_set_loop_warm_records says, unless the handle also opted in with qmpc_set_convex_warm_records below (plant records alone
 * follow the plain warm-started loop); a batch with no wrench-form kernel
 * under the handle's knobs with ctrl; a handle whose knot spacing is not the controller period of 5 ms (as qmpc_loop_run*).
 * Memory: the calls without outcome records run the outcome step on a scratch of 128 B x max_batch the handle allocates with
 * their other buffers.  QMPC_BAD_ARGUMENT for a null handle or another value; qmpc_query(QMPC_QUERY_CONVEX_RECORDS) returns
 * the setting. */
qmpc_status qmpc_set_convex_records(qmpc_handle* h, int32_t on);

/* Opt in to the lane-per-instance form of ConvexMpc's calls with per-instance records: on = 1 (0, the default, restores the
 * wave form at every size).  It holds until changed and takes effect only under qmpc_set_instances_policy(h,
 * QMPC_INSTANCES_AUTO), on a ConvexMpc handle in the converged mode that has a slot of the lane kernel's parameter table; the
 * setting does nothing on a handle of another model.
 *   qmpc_convex_solve_instances*: from the measured switch-over on (24576 instances at N <= 12, 26624 beyond; the knob
 *     QMPC_LANE_CINST_MIN overrides it, QMPC_VARIANT=4 takes the lane form at every size) the call runs
 *     qmpc_lane_cinst_kernel -- the passes of the plain ConvexMpc lane kernel with the record's fields read per LANE from a
 *     parameter block laid out like the lane workspace.  No lane pairs, no iteration cap, no hand-off: QMPC_KERNEL_LANE.  The
 *     results belong to the lane kernel's rounding family: bit-identical to qmpc_convex_solve's lane results on a handle that
 *     carries the same values (forces, info, trajectories), within 1e-7 N of the wave form's, status words equal.  Below the
 *     switch-over the wave form, bit for bit.  Measured at N=10, random records: 3.5 M solves/s at 32768 and 5.8 M at 65536
 *     instances, where the wave form does 2.7 / 2.8 M and the plain lane solve 3.9 / 6.5 M.
 *   qmpc_loop_run_instances* / _outcomes* / _pushes* with ctrl, on a handle that also opted in with qmpc_set_convex_records:
 *     cold-started per-tick calls from the larger of that switch-over and the plain cold loop's own take the lane form in every
 *     tick -- the sort (stance mask, the previous record's iteration class, robots that will not solve last) and
 *     qmpc_lane_cinst_kernel; with records equal to the handle's values the bytes of the plain ConvexMpc loop's lane tick.
 *     Persistent-kernel sizes stay persistent; the reference mode and a knot spacing other than 5 ms stay refused, and so
 *     does ctrl with lp->warm_start unless the handle opted in with qmpc_set_convex_warm_records below.
 * qmpc_query(QMPC_QUERY_KERNEL_FOR_CONVEX_INSTANCES / QMPC_QUERY_LOOP_INSTANCES_PLAN / QMPC_QUERY_LAST_KERNEL /
 * QMPC_QUERY_DEVICE_BYTES) answer under the setting and the policy, and qmpc_prepare_instances / qmpc_prepare allocate the
 * lane workspace, the sort scratch and 312 B per resident lane of parameter rows where the lane form is possible, so that a
 * caller's stream capture allocates nothing.  QMPC_BAD_ARGUMENT for a null handle or another value;
 * qmpc_query(QMPC_QUERY_CONVEX_LANE_RECORDS) returns the setting. */
qmpc_status qmpc_set_convex_lane_records(qmpc_handle* h, int32_t on);

/* Opt in to warm-started closed loops with controller records on a ConvexMpc handle: on = 1 (0, the default, restores the
 * refusal).  It holds until changed and takes effect only on a ConvexMpc handle in the converged mode that also opted in with
 * qmpc_set_convex_records; the setting does nothing on a handle of another model, and qmpc_set_loop_warm_records keeps having no
 * effect on ConvexMpc.  With both on, qmpc_loop_run_instances*, qmpc_loop_run_outcomes* and qmpc_loop_run_pushes* accept ctrl
 * together with lp->warm_start != 0, with the plain loop's rule: the first tick of a call starts cold, every later solve of a
 * robot starts from its previous solution shifted by one knot unless that solve failed (a frozen, halted or rejected robot never
 * solved).  Every other refusal keeps its code: the reference mode, a knot spacing other than 5 ms, no wrench-form kernel for
 * the batch, an 8-point handle.
 *   Launch (QMPC_QUERY_LOOP_INSTANCES_PLAN with bits 32 and 33 answers under the setting): the persistent kernel where the
 *     plain warm-started ConvexMpc loop takes its own on a wrench-form variant (up to 4096 robots, or QMPC_LOOP_FUSED);
 *     otherwise per tick -- the first tick qmpc_solve_cw_inst_kernel, the later ones qmpc_solve_cw_inst_warm_kernel, on the
 *     variant of qmpc_convex_solve_instances* for the batch.  On a handle that also opted in with qmpc_set_convex_lane_records,
 *     under QMPC_INSTANCES_AUTO, the per-tick calls take the lane form from the larger of its switch-over and the plain
 *     warm-started loop's own (QMPC_LANE_CINST_MIN / QMPC_LANE_MIN move them; QMPC_VARIANT=4: at every size): the sort and
 *     qmpc_lane_cinst_warm_kernel, after a first tick on qmpc_lane_cinst_kernel.  No lane pairs, no cap, no hand-off.
 *   With records equal to the handle's values every form gives the bytes of qmpc_loop_run* under the same lp (states, force and
 *     contact traces) wherever that loop solves in the same family on the same variant; the persistent and per-tick wave forms
 *     agree bit for bit on any records; wave and lane forms agree on status words and within 1e-7 N on forces.
 *   Memory: the per-tick forms carry the solution through a buffer of 96 N bytes per robot of max_batch.  qmpc_prepare,
 *     qmpc_prepare_instances and a call with ticks = 0 allocate it (and the lane buffers where the lane form is planned), so that
 *     a caller's stream capture allocates nothing; the persistent and per-tick wave forms run inside a caller's capture.
 * QMPC_BAD_ARGUMENT for a null handle or another value; qmpc_query(QMPC_QUERY_CONVEX_WARM_RECORDS) returns the setting. */
qmpc_status qmpc_set_convex_warm_records(qmpc_handle* h, int32_t on);

/* ---- per-robot outcome records of the closed loop (robustness sweeps) -------------------------------------------------
 * The other half of the question above: did robot i stay up, how far did it tilt, how well did it track its command, how
 * often was its solve rejected?  qmpc_loop_run_outcomes* is qmpc_loop_run_instances* -- the same robots, launch forms
 * (QMPC_QUERY_LOOP_INSTANCES_PLAN answers for it too), states and traces, bit for bit -- and accumulates one 128-byte record
 * per robot on the device inside the tick, instead of 6.5 KB of state per robot and tick crossing the link.
 *
 * A record is evaluated on the robot's state AFTER the post step of a tick: the new plant state, this tick's lin_vel_d_rel
 * and joy, the applied forces_body, status and iterations (loop_outcome_one, csrc/qmpc_loop_math.h: one source for the
 * device, the host class and the tests).  Minima and maxima skip non-finite values (a comparison with NaN selects nothing).
 * The robot is DOWN when pos_world[2] or the upright value is non-finite or below its threshold; the tick that leaves it
 * down is accumulated, then the record is frozen: down_tick is set and nothing further is added, in this call or a later one
 * with the same record.  Records are in/out and accumulate over calls: start from qmpc_loop_outcome_init.
 *
 * op->stop_when_down == 0: the robot is simulated on exactly as by qmpc_loop_run_instances*.  != 0: from the tick after its
 * down tick the robot is halted like the robot of an invalid record -- no solve runs for it (the persistent kernel's
 * wavefront leaves; in the per-tick form its input record gets a NaN attitude, which every solve kernel rejects before its
 * first iteration), its trace rows are zero -- and its state record is left untouched, so state.tick stays at down_tick.
 * A robot whose record comes in with down_tick >= 0 is halted from the first tick of the call.
 * The robot of an invalid controller or plant record (QMPC_BAD_PARAMS) leaves its outcome record untouched.
 *
 * Scope and refusals: those of qmpc_loop_run_instances* with records -- a QuatMpc handle in the converged mode, or a
 * ConvexMpc handle in the converged mode that opted in (qmpc_set_convex_records);
 * QMPC_UNSUPPORTED for a reference-mode handle or a ConvexMpc handle that has not opted in (qmpc_set_convex_records),
 * QMPC_BAD_ARGUMENT for an 8-point handle, with ctrl also
 * QMPC_UNSUPPORTED for lp->warm_start != 0 (unless the handle opted in: qmpc_set_loop_warm_records, ConvexMpc: qmpc_set_convex_warm_records) or a handle without a
 * wrench-form kernel -- and QMPC_BAD_ARGUMENT for a NULL op
 * or outcomes.  ctrl and plant may both be NULL: plain robots on the handle's parameters (still a QuatMpc converged
 * handle, or an opted-in ConvexMpc one).  Buffers: those of qmpc_loop_run_instances*; the host-buffer call adds a staging
 * buffer for the records (128 B x max_batch) on its first use.  No other call allocates it on a QuatMpc handle; an opted-in
 * ConvexMpc handle allocates it with the buffers of any call with records (qmpc_set_convex_records).  Under QMPC_INSTANCES_AUTO the ticks with ctrl take the lane
 * form of qmpc_loop_run_instances* from the same switch-over on; a halted robot then sorts into the class that will not
 * solve, so a fleet of which many are down runs in fewer wavefronts. */
typedef struct qmpc_outcome_params {   /* 4 doubles */
  double down_height;     /* default 0.15 m: down when pos_world[2] is below */
  double down_upright;    /* default 0.5 (cos of 60 deg tilt): down when the upright value is below */
  double stop_when_down;  /* 0 (default): go on simulating; != 0: halt the robot after its down tick */
  double reserved;        /* 0 */
} qmpc_outcome_params;
typedef struct qmpc_loop_outcome {     /* 16 doubles, 128 B; in/out: accumulates over calls */
  double ticks;               /* ticks accumulated into this record */
  double down_tick;           /* state.tick after the first tick that left the robot down; -1: never */
  double min_height;          /* min pos_world[2] */
  double min_upright;         /* min of the (3,3) entry of quat_to_rot(quat) = cos(tilt) */
  double max_height_err;      /* max |pos_world[2] - joy[2]| */
  double max_vel_err;         /* max e_v, e_v = |(R' lin_vel_world)_xy - lin_vel_d_rel_xy|_2 */
  double sum_vel_err_sq;      /* sum of e_v^2 (RMS = sqrt(sum / ticks)) */
  double max_ang_vel;         /* max |ang_vel_body|_inf */
  double max_force_z;         /* max over legs of the applied forces_body[3 leg + 2] */
  double not_ok_ticks;        /* ticks whose solve status != QMPC_OK */
  double rejected_ticks;      /* ticks whose solve was not applied (status neither QMPC_OK nor QMPC_MAX_ITER) */
  double first_rejected_tick; /* state.tick after the first such tick; -1: never */
  double iterations_sum, iterations_max;
  double reserved[2];         /* 0 */
} qmpc_loop_outcome;
void    qmpc_default_outcome_params(qmpc_outcome_params* op);
/* Host-side: `batch` empty records -- counters and sums 0, down_tick and first_rejected_tick -1, minima +inf, maxima -inf.
 * Every byte is written. */
void    qmpc_loop_outcome_init(qmpc_loop_outcome* outcomes, int32_t batch);
int32_t qmpc_sizeof_loop_outcome(void);
/* Host buffers: qmpc_loop_run_instances' arguments, then op and outcomes [batch] in/out.  Synchronous. */
qmpc_status qmpc_loop_run_outcomes(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                   int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                   double* trace_forces, double* trace_contacts, const qmpc_outcome_params* op,
                                   qmpc_loop_outcome* outcomes);
/* Device buffers (op is a host pointer, read during the call), stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_outcomes_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                          qmpc_loop_state* d_states, int32_t ticks,
                                          const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                          double* d_trace_forces, double* d_trace_contacts,
                                          const qmpc_outcome_params* op, qmpc_loop_outcome* d_outcomes, void* stream);

/* ---- timed push disturbances per robot (push recovery sweeps) ----------------------------------------------------------
 * The plant's disturbance wrench is constant over a call; a push needs a window in time.  qmpc_loop_run_pushes* is
 * qmpc_loop_run_outcomes* -- the same robots, launch forms (QMPC_QUERY_LOOP_INSTANCES_PLAN answers for it too), states,
 * traces, outcome records, halting and freezing -- whose plant step integrates under the EFFECTIVE wrench of the tick.  Each
 * robot carries pushes_per_robot windows: robot i's are push[i * pushes_per_robot + k].  The controller is not told.
 *
 * Window k acts in the tick that takes state.tick from t to t + 1 when t >= start_tick and t < start_tick + ticks (plain
 * double comparisons: fractional values are legal and only shift where they flip; ticks <= 0 never acts).  state.tick is
 * absolute, so a window spans calls: one call of T ticks equals calls of T1 + T2 ticks with the same records.
 *
 * Effective wrench, per component: start from the plant record's constant value (0 without plant records) and walk the
 * windows in index order.  An active window whose component is not exactly zero REPLACES the running value when that is
 * exactly zero and is ADDED to it with one IEEE add otherwise; an inactive window or an exactly zero component adds no
 * arithmetic (the rule of the plant's own disturbance; loop_push_wrench, csrc/qmpc_loop_math.h: one source for the device,
 * the host class and the tests).  So records that never act give the bytes of qmpc_loop_run_outcomes*, and one window over
 * the whole run on a plant without constant disturbance gives the bytes of that plant with the wrench as its disturbance.
 *
 * push == NULL: pushes_per_robot is ignored and the call IS qmpc_loop_run_outcomes*.  A robot one of whose windows has a
 * non-finite field is frozen with QMPC_BAD_PARAMS exactly like the robot of an invalid plant record: state untouched except
 * status and iterations, zero trace rows, outcome record untouched, every other robot unaffected bit for bit.
 * Call level: QMPC_BAD_ARGUMENT for a non-NULL push with pushes_per_robot outside 1 .. QMPC_MAX_PUSHES; everything else is
 * the outcome call's refusal, unchanged.  Buffers: those of qmpc_loop_run_outcomes*; the device call reads d_push in place;
 * the host-buffer call stages the windows in a buffer of its own (64 B x pushes_per_robot x max_batch), allocated on its
 * first use -- a call with ticks = 0 included -- and grown when pushes_per_robot grows.  No other call allocates it. */
#define QMPC_MAX_PUSHES 8
typedef struct qmpc_push_params {   /* 8 doubles, 64 B: one push window of one robot */
  double start_tick;        /* first tick it acts in, counted in state.tick (absolute: carries over calls) */
  double ticks;             /* length of the window in ticks; <= 0: no push */
  double force_world[3];    /* at the CoM, world frame [N] */
  double torque_body[3];    /* body frame [N m] */
} qmpc_push_params;
int32_t qmpc_sizeof_push_params(void);
/* Host buffers: qmpc_loop_run_outcomes' arguments, then push [batch][pushes_per_robot].  Synchronous. */
qmpc_status qmpc_loop_run_pushes(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                 int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                 double* trace_forces, double* trace_contacts, const qmpc_outcome_params* op,
                                 qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int32_t pushes_per_robot);
/* Device buffers (op is a host pointer, read during the call), stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_pushes_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                        qmpc_loop_state* d_states, int32_t ticks,
                                        const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                        double* d_trace_forces, double* d_trace_contacts,
                                        const qmpc_outcome_params* op, qmpc_loop_outcome* d_outcomes,
                                        const qmpc_push_params* d_push, int32_t pushes_per_robot, void* stream);

/* ---- per-robot ground friction and force limits in the plant (the true ground under each foot) -------------------------
 * The controller records carry a friction coefficient and a normal-force bound; the plant above delivers whatever force the
 * solve returns.  qmpc_loop_run_ground* is qmpc_loop_run_pushes* -- the same robots, launch forms
 * (QMPC_QUERY_LOOP_INSTANCES_PLAN answers for it too), refusals, ticks = 0 behaviour, freezing and halting -- whose plant
 * integrates under the force the robot's TRUE ground delivers.  The controller is not told.
 *
 * In the back end of a tick, after grf_world has been formed as always (QuatMpc: R forces_body; ConvexMpc: the solve's
 * world-frame forces), every leg with contacts[l] != 0 of a robot whose record has at least one finite field is clamped on
 * its world-frame force f = (fx, fy, fz), in this order (loop_ground_leg, csrc/qmpc_loop_math.h: one source for the device,
 * the host class and the tests):
 *   1. fz < 0: f = 0 (the ground does not pull); counted as normal
 *   2. fz > fz_max[l]: fz = fz_max[l]; counted as normal
 *   3. t = sqrt(fx fx + fy fy) > mu[l] fz: fx and fy are multiplied by s = (mu[l] fz) / t; counted as friction (mu = 0 gives
 *      zeros of either sign)
 * A leg no rule changed keeps its bytes -- no arithmetic, no `+ 0.0`; swing legs are not looked at.  The plant step takes the
 * delivered body-frame force R' f of a changed leg and the commanded forces_body bytes of an unchanged one, under the tick's
 * effective wrench (pushes compose).  state.grf_world holds the DELIVERED force; state.forces_body and trace_forces stay
 * the controller's COMMAND (what tau = -J' f and the outcome record's max_force_z read, what a warm start continues from).
 * (A ConvexMpc tick whose solve was rejected clamps R forces_body, the command the plant keeps applying.)
 * So ground == NULL, an all-+inf record and a finite record that never binds give the bytes of qmpc_loop_run_pushes*.
 * (Never binds is a statement about the forces too: a stance leg whose command is the solver's zero arrives as +-1e-15 N per
 * component, and a finite record binds there on a negative fz or on |f_xy| > mu fz; an all-+inf record looks at no leg.)
 *
 * tally (may be NULL) accumulates over calls like the outcome records, from the same verdicts; a robot that is frozen or
 * halted leaves its tally untouched.  Start from qmpc_ground_tally_init.
 *
 * A record with a NaN field, a mu < 0 or an fz_max <= 0 makes its robot the robot of an invalid plant record
 * (QMPC_BAD_PARAMS: state untouched except status and iterations, zero trace rows, outcome record and tally untouched, every
 * other robot unaffected bit for bit).  ground == NULL: the call IS qmpc_loop_run_pushes* and tally is not touched.  push may be
 * NULL (no windows; pushes_per_robot ignored).  Buffers: those of the push call; the device call reads d_ground in place;
 * the host-buffer call stages records and tallies in a buffer of its own ((64 + 32) B x max_batch), allocated on its first
 * use -- a call with ticks = 0 included.  No other call allocates it. */
typedef struct qmpc_ground_params {   /* 8 doubles, 64 B: the TRUE ground / actuator under each foot */
  double mu[4];       /* Coulomb coefficient under leg l; +inf: no limit; 0 legal (ice) */
  double fz_max[4];   /* largest normal force leg l can receive [N]; +inf: no limit */
} qmpc_ground_params;
typedef struct qmpc_ground_tally {    /* 4 doubles, 32 B; in/out: accumulates over calls */
  double clipped_ticks;          /* ticks in which the delivered force of >= 1 stance leg differs from the command */
  double first_clipped_tick;     /* state.tick after the first such tick; -1: never */
  double friction_leg_ticks;     /* (leg, tick) pairs whose tangential force was scaled down */
  double normal_leg_ticks;       /* (leg, tick) pairs whose normal force was cut (above fz_max, or negative) */
} qmpc_ground_tally;
/* Host-side; every byte is written: every field +inf / 0, -1, 0, 0 */
void    qmpc_ground_params_init(qmpc_ground_params* g, int32_t batch);
void    qmpc_ground_tally_init(qmpc_ground_tally* t, int32_t batch);
int32_t qmpc_sizeof_ground_params(void);
int32_t qmpc_sizeof_ground_tally(void);
/* Host buffers: qmpc_loop_run_pushes' arguments, then ground [batch] and tally [batch] in/out (or NULL).  Synchronous. */
qmpc_status qmpc_loop_run_ground(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                 int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                 double* trace_forces, double* trace_contacts, const qmpc_outcome_params* op,
                                 qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int32_t pushes_per_robot,
                                 const qmpc_ground_params* ground, qmpc_ground_tally* tally);
/* Device buffers (op is a host pointer, read during the call), stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_ground_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                        qmpc_loop_state* d_states, int32_t ticks,
                                        const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                        double* d_trace_forces, double* d_trace_contacts,
                                        const qmpc_outcome_params* op, qmpc_loop_outcome* d_outcomes,
                                        const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                        const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally, void* stream);

/* ---- actuation delay and actuator lag per robot (time between the solve and the force under the feet) -------------------
 * In every loop above the force solved from the state at tick t acts on the plant during tick t: no compute latency, infinite
 * actuator bandwidth.  qmpc_loop_run_actuation* is qmpc_loop_run_ground* -- the same robots, launch forms
 * (QMPC_QUERY_LOOP_INSTANCES_PLAN answers for it too), refusals, ticks = 0 behaviour, freezing, halting and ConvexMpc opt-ins
 * -- whose plant receives the command of delay_ticks ticks ago through a first-order actuator.  The controller is not told.
 *
 * The rule (loop_actuation_one, csrc/qmpc_loop_math.h: one source for the device, the host class and the tests) runs in the
 * back end of a tick, after state.forces_body holds this tick's command c by the accept / reject rule of every loop (a
 * rejected solve keeps the last accepted command, and that command is what is pushed):
 *   1. push     line.cmd[count mod QMPC_MAX_DELAY] = c, copied as bytes
 *   2. target   y = the slot of command number count - delay_ticks when that number is >= 0; otherwise the line predates the
 *               first command and y is slot (count - delay_ticks) mod QMPC_MAX_DELAY taken non-negative, which still holds
 *               the initial force qmpc_actuation_line_init wrote.  delay_ticks = 0: y is the bytes of c.  (delay_ticks =
 *               QMPC_MAX_DELAY reads the slot before step 1 overwrites it.)
 *   3. lag      per component: alpha == 1: a = y as bytes, no arithmetic; otherwise a = applied + alpha * (y - applied) --
 *               one subtract, one multiply, one add, in that order
 *   4. swing    a leg with contacts[l] == 0 delivers exactly +0.0 in all three components and its applied becomes +0.0: an
 *               unloaded leg cannot push, and its actuator starts from rest at touchdown
 *   5. store    applied = a, then count += 1
 * A robot whose record is the identity (delay_ticks = 0, alpha = 1) takes the ground call's post step as it stands (QuatMpc:
 * grf_world = R forces_body; ConvexMpc: the solve's world-frame bytes); steps 1 and 5 still keep its line current, so its
 * state, traces, outcome record and tally are the bytes of qmpc_loop_run_ground*.  Any other robot forms grf_world = R a (in
 * the expression shape of R forces_body; a swing leg's entry is +0.0) and passes through the ground clamp unchanged: a
 * changed leg hands the plant R' f, an unchanged one a.  The plant steps under those twelve values and the tick's effective
 * wrench, so pushes and ground compose.  state.forces_body and trace_forces stay the controller's COMMAND (what a warm start
 * continues from, what tau = -J' f and the outcome record's max_force_z read); state.grf_world holds the DELIVERED force.
 *
 * act == NULL: the call IS qmpc_loop_run_ground* and line is not touched.  act != NULL with line == NULL: QMPC_BAD_ARGUMENT.
 * ground == NULL with act != NULL: no clamp -- the bytes an all-+inf ground record gives; tally is untouched and no ground
 * record is read.  A record with a non-finite field, a delay_ticks that is not an integer in 0 .. QMPC_MAX_DELAY, an alpha
 * outside (0, 1], or a line whose count is negative, non-integer, non-finite or beyond 2^53 makes its robot the robot of an
 * invalid plant record (QMPC_BAD_PARAMS, marked by a check kernel before the first tick: state untouched except status and
 * iterations, zero trace rows, outcome record, tally and line untouched, every other robot unaffected bit for bit).  A frozen
 * or halted robot leaves its line untouched.  Buffers: those of the ground call; the device call reads d_act and works on
 * d_line in place; the host-buffer call stages records and lines in a buffer of its own ((32 + 896) B x max_batch), allocated
 * on its first use -- a call with ticks = 0 included.  No other call allocates it. */
#define QMPC_MAX_DELAY 8
typedef struct qmpc_actuation_params {   /* 4 doubles, 32 B */
  double delay_ticks;   /* 0 .. QMPC_MAX_DELAY, integer-valued: the plant receives the command of delay_ticks ticks ago */
  double alpha;         /* first-order actuator response per tick, in (0, 1]; exactly 1: none.  alpha = 1 - exp(-dt / tau) */
  double reserved[2];   /* 0 */
} qmpc_actuation_params;
typedef struct qmpc_actuation_line {     /* 112 doubles, 896 B; in/out: the robot's delay line, carries over calls */
  double cmd[QMPC_MAX_DELAY][12];  /* ring of body-frame commands; the command number c sits in slot c mod QMPC_MAX_DELAY */
  double applied[12];              /* body-frame force the actuators produced in the last tick (the lag's state) */
  double count;                    /* commands pushed so far (integer-valued, >= 0) */
  double reserved[3];
} qmpc_actuation_line;
/* Host-side; every byte is written.  The identity record (delay_ticks = 0, alpha = 1); every ring slot and applied hold
 * initial_forces_body ([12], or NULL = zeros), count = 0 */
void    qmpc_actuation_params_init(qmpc_actuation_params* act, int32_t batch);
void    qmpc_actuation_line_init(qmpc_actuation_line* line, int32_t batch, const double* initial_forces_body);
int32_t qmpc_sizeof_actuation_params(void);
int32_t qmpc_sizeof_actuation_line(void);
/* Host buffers: qmpc_loop_run_ground's arguments, then act [batch] and line [batch] in/out.  Synchronous. */
qmpc_status qmpc_loop_run_actuation(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                    int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                    double* trace_forces, double* trace_contacts, const qmpc_outcome_params* op,
                                    qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int32_t pushes_per_robot,
                                    const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                                    const qmpc_actuation_params* act, qmpc_actuation_line* line);
/* Device buffers (op is a host pointer, read during the call), stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_actuation_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                           qmpc_loop_state* d_states, int32_t ticks,
                                           const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                           double* d_trace_forces, double* d_trace_contacts,
                                           const qmpc_outcome_params* op, qmpc_loop_outcome* d_outcomes,
                                           const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                           const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                           const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line, void* stream);

/* ---- state-estimate bias and noise per robot (what the controller reads is not what the plant is) -----------------------
 * In every loop above the controller reads the plant's true state to the last bit.  qmpc_loop_run_sensing* is
 * qmpc_loop_run_actuation* -- the same robots, launch forms (QMPC_QUERY_LOOP_INSTANCES_PLAN answers for it too), refusals,
 * ticks = 0 behaviour, freezing, halting, ConvexMpc and warm-record opt-ins -- whose controller reads a MEASURED state: the
 * true pos_world, quat, lin_vel_world and ang_vel_body plus a per-robot bias and per-robot, per-tick, reproducible bounded
 * noise.  The plant, the outcome record, pushes, ground and actuation keep working on the truth.
 *
 * The rule (loop_sense_one, csrc/qmpc_loop_math.h: one source for the device, the host class and the tests), in the front
 * end of the tick that starts at t = (uint64) state.tick:
 *   noise    for channel c in 0 .. 11:  z = mix(seed + 0x9E3779B97F4A7C15 * (12 t + c + 1)), wrapping in 64 bits, mix the
 *            splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *            z ^= z >> 31);  S = the sum of the four 16-bit fields of z;  n = (double)(int)(S - 131070) * 0x1.bb67ae86627e7p-16
 *            (the constant is 1 / sqrt((2^32 - 1) / 3)).  n is an Irwin-Hall(4) variate: mean 0, variance 1, close to a normal
 *            one in the middle and BOUNDED by +-3.4641 (2 sqrt 3) -- for a robustness sweep the bound is a feature: no run is
 *            decided by one sample from a far tail.  Integer-only up to one conversion and one multiply: no libm call, the same
 *            bits everywhere.  It is keyed on state.tick, not on the call: a run split over calls draws the same noise.
 *   error    e_c = bias[c] + sigma[c] * n_c.  A channel with sigma == 0 evaluates no hash (e_c = bias[c]); a channel with
 *            bias == 0 and sigma == 0 is inactive: it contributes no arithmetic, its field is copied as bytes.
 *   measure  position, velocity, body rate: m = x + e.  Attitude, if any of channels 3-5 is active: q_m = normalize(q (x)
 *            (1, phi / 2)), phi = e_3..5 (an inactive channel's entry 0), scalar first, Hamilton product with its terms summed
 *            left to right, the norm the sqrt of the four squares summed left to right, then four divisions.  That rotates by
 *            2 atan(|phi| / 2) about phi in the body frame -- |phi| to within |phi|^3 / 12 -- without sin or cos.  Otherwise
 *            the quaternion is copied as bytes.
 * foot_pos_world and the contact flags are not touched (the stance feet are what leg odometry anchors on, the flags come from
 * the feet): the controller's foot_pos_body becomes R_m' (foot - p_m).
 *
 * A robot whose record is the identity (all of bias and sigma zero; seed ignored) runs the front end as it stands; its seen
 * is untouched.  Any other robot saves the 13 true doubles, writes the measured ones into the state, runs the front end
 * unchanged, restores the 13 true doubles as bytes and writes seen when given.  Nothing else in the tick changes: the post step
 * (grf_world = R forces_body with the TRUE R), the plant, the outcome record, the ground clamp and the delay line see the truth.
 * Frozen and halted robots leave seen untouched.
 *
 * sense == NULL: the call IS qmpc_loop_run_actuation* and seen is not touched.  act may be NULL with sense given (line is then
 * ignored): every command reaches the plant in its own tick.  A record with a non-finite field, a sigma < 0 or a seed that is
 * not an integer in [0, 2^53) makes its robot the robot of an invalid plant record (QMPC_BAD_PARAMS, marked by a check kernel
 * before the first tick; every other robot unaffected bit for bit).  Buffers: those of the actuation call; the device call reads
 * d_sense and works on d_seen in place; the host-buffer call stages records and seen in a buffer of its own ((256 + 128) B x
 * max_batch), allocated on its first use -- a call with ticks = 0 included.  No other call allocates it. */
typedef struct qmpc_sense_params {   /* 32 doubles, 256 B: what robot i's estimator gets wrong */
  double bias[12];     /* channels 0-2 pos_world [m], 3-5 attitude error phi, body frame [rad],
                          6-8 lin_vel_world [m/s], 9-11 ang_vel_body [rad/s] (gyro bias) */
  double sigma[12];    /* standard deviation of the per-tick noise on the same channels, >= 0 */
  double seed;         /* integer-valued, 0 .. 2^53 - 1 */
  double reserved[7];  /* 0 */
} qmpc_sense_params;
typedef struct qmpc_sense_seen {     /* 16 doubles, 128 B; in/out, may be NULL */
  double meas[13];     /* pos[3] quat[4] lin_vel_world[3] ang_vel_body[3] the controller read in the robot's last tick */
  double ticks;        /* ticks in which a non-identity measurement was formed; accumulates over calls */
  double reserved[2];
} qmpc_sense_seen;
/* Host-side; every byte is written: the identity record (all zero), an empty seen (all zero) */
void    qmpc_sense_params_init(qmpc_sense_params* sense, int32_t batch);
void    qmpc_sense_seen_init(qmpc_sense_seen* seen, int32_t batch);
int32_t qmpc_sizeof_sense_params(void);
int32_t qmpc_sizeof_sense_seen(void);
/* Host buffers: qmpc_loop_run_actuation's arguments, then sense [batch] and seen [batch] in/out (or NULL).  Synchronous. */
qmpc_status qmpc_loop_run_sensing(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                  int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                  double* trace_forces, double* trace_contacts, const qmpc_outcome_params* op,
                                  qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int32_t pushes_per_robot,
                                  const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                                  const qmpc_actuation_params* act, qmpc_actuation_line* line,
                                  const qmpc_sense_params* sense, qmpc_sense_seen* seen);
/* Device buffers (op is a host pointer, read during the call), stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_sensing_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                         qmpc_loop_state* d_states, int32_t ticks,
                                         const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                         double* d_trace_forces, double* d_trace_contacts,
                                         const qmpc_outcome_params* op, qmpc_loop_outcome* d_outcomes,
                                         const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                         const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                         const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                                         const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen, void* stream);

/* ---- gait frequency and contact pattern per robot (which gait and cadence survives this shove?) -------------------------
 * In every loop above all robots of a call walk the reference's trot at lp->gait_freq.  qmpc_loop_run_gaits* is
 * qmpc_loop_run_sensing* -- the same arguments in their order, robots, launch forms (QMPC_QUERY_LOOP_INSTANCES_PLAN answers for
 * it too), refusals, ticks = 0 behaviour, freezing, halting, ConvexMpc and warm-record opt-ins, the lane tick under
 * QMPC_INSTANCES_AUTO -- with one more record per robot before `stream`: its gait.  It adds no in/out record: the schedule
 * lives in qmpc_loop_state::leg[], contacts and gait_counter, as it always did.
 *
 * The reference's FSM holds a pattern of states and switch times per leg; its update() toggles the state on every transition
 * instead of reading the pattern, so only two-entry patterns work as written.  A robot's gait here is therefore, per leg, a
 * two-entry pattern -- [STANCE, SWING] or [SWING, STANCE] with switch times split and 1.0 -- plus the phase the leg starts at.
 *
 * The rule (loop_gait_* in csrc/qmpc_loop_math.h: one source for the device, the host classes and the tests):
 *   pattern   pattern(leg, idx) = ((idx == 0) == (first_stance[leg] != 0)) ? STANCE : SWING; switch_time(leg, idx) = idx == 0 ?
 *             split[leg] : 1.0.
 *   update    the reference's update / common_enter (LeggedContactFSM.cpp:33-78,208-223) with gait_freq and the switch times of
 *             the record; the early-contact branch (percent > 0.9 and the contact flag) is unchanged.
 *   reset     every tick while movement_mode == 0, and in qmpc_loop_state_set_gait:  gait_phase = phase0;  idx = phase0 < split ?
 *             0 : 1;  pattern_index = idx, prev_pattern_index = 1 - idx;  start_time = idx ? split : 0, end_time = idx ? 1 : split;
 *             state = pattern(idx); everything else as the reference's reset().  With phase0 = 0 these are the trot's bytes.
 *   swing     the reference's literal 0.5 in the swing curve's times is the trot's swing fraction; a leg uses its own,
 *             w = first_stance ? 1 - split : split:  swing target at (float)(w t / f) of (float)(w / f).
 *   Raibert   the literal (1 / f) / 2 is the trot's stance time; a leg uses (1 / f) (1 - w), the +-0.5 / +-0.3 clamps per leg.
 *             At w = 1/2 both give the trot's bits (a scaling by a power of two is exact).
 *
 * A record is the IDENTITY when gait_freq == lp->gait_freq, first_stance == {1, 0, 0, 1}, every split == 0.5 and every
 * phase0 == 0: its robot, and every robot when gait == NULL, runs the front end of the sensing call as it stands -- every byte
 * equals that call's.  gait == NULL: the call IS qmpc_loop_run_sensing*.  Every other record may be NULL as in that call.
 *
 * A record is VALID when every field is finite and the reserved words are 0; gait_freq > 0 and gait_freq * lp->dt <= 1/16 (every
 * arc lasts at least two ticks); first_stance is 0 or 1; split is a multiple of 2^-8 in [1/8, 7/8]; phase0 a multiple of 2^-8 in
 * [0, 1); and the schedule plans no flight: with the leg's stance arc in the robot's phase starting at A = frac(a - phase0 + 1)
 * (a = 0 or split) with length len (split or 1 - split), the end frac(A + len) of every leg's arc lies in some leg's arc
 * (frac(E - A_m + 1) < len_m) -- exact arithmetic on dyadic numbers.  Pronk and every gait with a flight phase are refused.  An
 * invalid record makes its robot the robot of an invalid plant record (QMPC_BAD_PARAMS, marked by a check kernel after the
 * sensing check; every other robot unaffected bit for bit).  A tick without a stance leg can still happen by a rounding
 * coincidence of two legs' phase accumulators, as in the trot after an early contact: it ends as there (QMPC_NO_CONTACT, the
 * last forces stay).
 *
 * Between calls: split and gait_freq take effect at each leg's next transition, phase0 only at a reset -- a run split into
 * calls with different records is a gait transition.  Buffers: those of the sensing call; the host-buffer call stages the
 * records in a buffer of its own (128 B x max_batch), allocated on its first use.  No other call allocates it. */
typedef struct qmpc_gait_params {   /* 16 doubles, 128 B */
  double gait_freq;        /* cycles per second, replaces lp->gait_freq for this robot */
  double first_stance[4];  /* 1: the leg's pattern is [STANCE, SWING]; 0: [SWING, STANCE] */
  double split[4];         /* the leg's first switch time; the second is 1.0 */
  double phase0[4];        /* the leg's gait_phase at an FSM reset */
  double reserved[3];      /* must be 0 */
} qmpc_gait_params;
int32_t qmpc_sizeof_gait_params(void);
/* Host-side; every byte is written: the identity record of lp (the reference's trot at lp->gait_freq) */
void    qmpc_default_gait_params(const qmpc_loop_params* lp, qmpc_gait_params* out);
/* Host-side: the reset rule above on the four legs of s, and contacts = the legs' states.  After qmpc_loop_state_init, for a
 * robot that walks (movement_mode != 0) from tick 0 in the gait's own pattern.  The record is not checked. */
void    qmpc_loop_state_set_gait(qmpc_loop_state* s, const qmpc_gait_params* gait);
/* The contact schedule a robot's gait state implies over a horizon: masks[k], k = 0 ... N-1, bit l set where leg l stands during
 * knot k -- a row of qmpc_solve_schedule*'s schedule.  Host-side, no GPU involved.  masks[0] is s->contacts as it stands; then a
 * copy of each leg's gait_phase, state, pattern_index, start_time and end_time is advanced N - 1 times by gait_freq * h with the
 * schedule step of the loop's tick (the stance exit at end_time, the swing exit at the end of the swing arc, the pattern's
 * next entry), without early contacts and without the swing trajectory, one mask after each advance.  *s is not changed.
 * g == NULL: the reference's trot at lp->gait_freq (qmpc_default_gait_params); otherwise lp may be NULL.  h: the knot spacing
 * (the handle's params.h).  Nothing is written for a null s or masks, N < 1, or g and lp both null.
 * For a leg the schedule lands inside the horizon the caller of qmpc_solve_schedule* puts the touchdown point into
 * qmpc_input::foot_pos_body[l]: the leg's foot_target_world, taken to the body frame like the other feet.  (The closed loops do
 * not call this yet.) */
void    qmpc_gait_predict(const qmpc_loop_params* lp, const qmpc_gait_params* g, const qmpc_loop_state* s, double h, int32_t N,
                          uint8_t* masks);
/* Host buffers: qmpc_loop_run_sensing's arguments, then gait [batch] (or NULL).  Synchronous. */
qmpc_status qmpc_loop_run_gaits(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                double* trace_forces, double* trace_contacts, const qmpc_outcome_params* op,
                                qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int32_t pushes_per_robot,
                                const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                                const qmpc_actuation_params* act, qmpc_actuation_line* line,
                                const qmpc_sense_params* sense, qmpc_sense_seen* seen, const qmpc_gait_params* gait);
/* Device buffers (op is a host pointer, read during the call), stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_gaits_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                       qmpc_loop_state* d_states, int32_t ticks,
                                       const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                       double* d_trace_forces, double* d_trace_contacts,
                                       const qmpc_outcome_params* op, qmpc_loop_outcome* d_outcomes,
                                       const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                       const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                       const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                                       const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen,
                                       const qmpc_gait_params* d_gait, void* stream);

/* ---- motor torque limits and joint torque peaks per robot (which motor is too small; what torque does this fleet need?) ----
 * The only actuator limit above is qmpc_ground_params::fz_max, a cap on a foot's normal force that knows nothing of the leg's
 * posture.  A robot's motors saturate in joint torque.  qmpc_loop_run_motors* is qmpc_loop_run_gaits* -- the same arguments in
 * their order, robots, launch forms (QMPC_QUERY_LOOP_INSTANCES_PLAN answers for it too), refusals, ticks = 0 behaviour,
 * freezing, halting, ConvexMpc and warm-record opt-ins, the lane tick under QMPC_INSTANCES_AUTO -- with three more arguments
 * before `stream`: geom (a HOST pointer in both calls, read during the call like op; one geometry for all robots; NULL:
 * qmpc_default_go1_geometry), per robot a motor record, and per robot a tally, in/out, that accumulates over calls and is
 * required when motor is given (QMPC_BAD_ARGUMENT otherwise).  motor == NULL: the call IS qmpc_loop_run_gaits*.
 *
 * The rule (loop_motor_* in csrc/qmpc_joint_math.h: one source for the device, the host class and the tests) runs in the post
 * step of a tick, after the body-frame force u that the actuators produce is known (forces_body, or with an actuation record
 * what the delay line and lag return) and before the ground clamp and the plant step, on R, pos_world and foot_pos_world as
 * they are there -- the pose before the plant step:
 *   angles    every leg, every tick: pb = R'(foot - p); q = the closed-form inverse kinematics of pb with the hip branch
 *             nearest joint_pos[3l].  A NaN in q keeps the previous angles and adds 1 to unreachable_leg_ticks (the rule of
 *             qmpc_loop_joint_commands).  joint_pos takes q.
 *   demand    stance legs only (contacts[l] != 0; a swing leg delivers nothing and is not looked at): J = the leg Jacobian at
 *             q, tau_j = -(J[3j] u0 + J[3j+1] u1 + J[3j+2] u2); peak_tau[3l+j] = max(peak_tau[3l+j], |tau_j|).
 *   clip      if no |tau_j| > tau_max[3l+j] the leg is untouched -- no arithmetic reaches its bytes; equality does not bind, a
 *             +inf limit never binds.  Otherwise t_j = copysign(tau_max, tau_j) on the binding joints and tau_j on the others,
 *             sat_ticks of each binding joint gets +1, and u' solves J' u' = -t (a pivoted 3x3 elimination).  If a component of
 *             u' is not finite (a singular leg) the leg stays untouched and unreachable_leg_ticks gets +1; otherwise the leg
 *             delivers u'.
 *   changed   a leg the motor changed gets grf_world[l] = R u' before the ground clamp sees it; the plant receives u', or R' f
 *             if the ground changes the leg too.  A leg it did not change keeps exactly what the gaits call gives it.
 *   fields    forces_body and the trace row hold the command, grf_world the delivered force.  The actuation line's `applied`
 *             is not touched: the lag is inside the motor, the clip comes after it.  Outcome records, pushes, sensing and gaits
 *             read what they read in the gaits call.
 *   tally     if any leg was changed in the tick clipped_ticks gets +1 and first_clipped_tick is set once, to state.tick after
 *             the tick.
 *
 * A record is VALID when every tau_max > 0 (+inf passes, NaN fails) and the reserved words are 0; a tally when its joint_pos is
 * finite and its counters (sat_ticks, clipped_ticks, unreachable_leg_ticks) are non-negative integers below 2^53.  An invalid
 * one makes its robot the robot of an invalid plant record (QMPC_BAD_PARAMS, marked by a check kernel after the gait check; its
 * tally untouched, every other robot unaffected bit for bit).
 *
 * IDENTITY: with every limit +inf the robot's state, outcome record, ground tally, delay line, seen and trace rows are the
 * gaits call's bytes in every launch form; joint_pos and peak_tau are still filled in -- the "what torque does this need" use.
 *
 * Buffers: those of the gaits call; the host-buffer call stages records and tallies in a buffer of its own ((128 + 320) B x
 * max_batch), allocated on its first use (by ticks = 0 too) and counted in QMPC_QUERY_DEVICE_BYTES.  No other call allocates it.
 * Not modelled: torque-speed derating, a geometry per robot, joint position limits.  The 8-point model and the reference mode
 * are refused exactly as the gaits call refuses them. */
typedef struct qmpc_motor_params {   /* 16 doubles, 128 B */
  double tau_max[12];      /* N m, leg-major (hip, thigh, calf); +inf: no limit */
  double reserved[4];      /* must be 0 */
} qmpc_motor_params;
typedef struct qmpc_motor_tally {    /* 40 doubles, 320 B; in/out, accumulates over calls */
  double joint_pos[12];    /* the hip-branch memory of the inverse kinematics; start: the stand pose of qmpc_loop_joint_init */
  double peak_tau[12];     /* the largest |torque| demanded of the joint while its leg stood, before clipping */
  double sat_ticks[12];    /* the ticks the joint was clipped */
  double clipped_ticks;    /* the ticks in which the motors changed a leg */
  double first_clipped_tick;     /* state.tick after the first such tick; -1 until then */
  double unreachable_leg_ticks;  /* leg-ticks with a foot out of reach or a singular leg under a binding limit */
  double reserved;
} qmpc_motor_tally;
int32_t qmpc_sizeof_motor_params(void);
int32_t qmpc_sizeof_motor_tally(void);
/* Host-side; every byte is written: every limit +inf, reserved 0 */
void    qmpc_default_motor_params(qmpc_motor_params* out);
/* Host-side; every byte is written: joint_pos the stand pose, first_clipped_tick -1, everything else 0 */
void    qmpc_motor_tally_init(qmpc_motor_tally* out);
/* Host buffers: qmpc_loop_run_gaits's arguments, then geom (or NULL), motor [batch] (or NULL), tally [batch].  Synchronous. */
qmpc_status qmpc_loop_run_motors(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                 int32_t ticks, const qmpc_instance_params* ctrl, const qmpc_plant_params* plant,
                                 double* trace_forces, double* trace_contacts, const qmpc_outcome_params* op,
                                 qmpc_loop_outcome* outcomes, const qmpc_push_params* push, int32_t pushes_per_robot,
                                 const qmpc_ground_params* ground, qmpc_ground_tally* tally,
                                 const qmpc_actuation_params* act, qmpc_actuation_line* line,
                                 const qmpc_sense_params* sense, qmpc_sense_seen* seen, const qmpc_gait_params* gait,
                                 const qmpc_leg_geometry* geom, const qmpc_motor_params* motor, qmpc_motor_tally* motor_tally);
/* Device buffers (op and geom are host pointers, read during the call), stream-ordered (NULL stream = the handle's). */
qmpc_status qmpc_loop_run_motors_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                        qmpc_loop_state* d_states, int32_t ticks,
                                        const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                        double* d_trace_forces, double* d_trace_contacts,
                                        const qmpc_outcome_params* op, qmpc_loop_outcome* d_outcomes,
                                        const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                        const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                        const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                                        const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen,
                                        const qmpc_gait_params* d_gait, const qmpc_leg_geometry* geom,
                                        const qmpc_motor_params* d_motor, qmpc_motor_tally* d_motor_tally, void* stream);

/* Stand-pose joint angles (0, 0.67, -1.3 per leg: the reference's Gazebo start pose) for `batch`
 * robots, host buffer [batch][12]. */
void qmpc_loop_joint_init(double* joint_pos, int32_t batch);

/* ---- diagnostics ----------------------------------------------------------- */
/* C = X' * Y on [12][16] row-major tiles through the FP64 MFMA path the solver
 * uses (host buffers of 192 doubles each).  Lets the GPU tests pin the
 * fragment layout independently of the solver. */
qmpc_status qmpc_selftest_mtm(int32_t device, const double* X, const double* Y, double* C);
/* Cross-lane primitives of the stage solve on 64 doubles: out = 9 x 64 doubles
 * (row-group broadcasts 0..3, wave sum / max / min, row_newbcast:5, quad_perm[1,1,1,1]). */
qmpc_status qmpc_selftest_lanes(int32_t device, const double* in, double* out);
/* Per-instance phase cycle counts (s_memtime) of one instrumented solve launch:
 * cycles_out [batch][16] int64 (host); slots 0..14 = set-up, expansions, operand
 * build, MFMA + stage terms, stage solve, cost-to-go update, IPM directions,
 * rollout (rest), misc, rotation pre-pass, rollout gain / broadcast / step,
 * apply, wait for the last products; slot 15 = iterations.  Used by
 * tools/phase_profile.py. */
qmpc_status qmpc_debug_profile(qmpc_handle* h, int32_t batch, const qmpc_input* in, int64_t* cycles_out);

/* ---- introspection -------------------------------------------------------- */
const char* qmpc_status_string(int32_t status);
const char* qmpc_version(void);
int32_t     qmpc_sizeof_input(void);   /* ABI guards for foreign-language bindings */
int32_t     qmpc_sizeof_params(void);
int32_t     qmpc_sizeof_info(void);
int32_t     qmpc_sizeof_convex_input(void);
int32_t     qmpc_sizeof_input8(void);

#ifdef __cplusplus
}
#endif
#endif /* QMPC_H_ */
