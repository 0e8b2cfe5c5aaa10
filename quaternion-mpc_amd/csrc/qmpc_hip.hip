// qmpc_hip.hip -- C ABI (include/qmpc.h) over the gfx950 kernels.
//
// Drop-in boundary: replaces the ALTRO set-up / Solve() / GetInput(0) block of
// legged::QuatMpc::grf_update (legged_ctrl/src/mpc/QuatMpc.cpp:217-265) -- and, for
// handles created with params.model = QMPC_MODEL_CONVEX, of legged::ConvexMpc::grf_update
// (legged_ctrl/src/mpc/ConvexMpc.cpp:84-186) -- for a batch of independent LeggedState
// records.  No CPU fallback exists here: with no HIP device every entry point returns
// QMPC_NO_DEVICE.
#include "qmpc_kernels.hip"
#include "qmpc_loop.hip"
#include "qmpc_joint.hip"
#include "qmpc_ref.hip"

#include <dlfcn.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>

#include "qmpc_kernel_slots.h"
#include "qmpc_loop_records.h"
#include "qmpc_plan_fill.h"

using namespace qmpc;

// the launch tables of this unit (slots: qmpc_kernel_slots.h): the round-1 solve kernels (the profiling ones included), the
// reference mode's and the linearisation
static decltype(&qmpc_solve_kernel<QuatModel, false, 0>) const kDenseSolve[] = {
    qmpc_solve_kernel<QuatModel, false, 0>,   qmpc_solve_kernel<QuatModel, false, 1>,   qmpc_solve_kernel<QuatModel, false, 2>,
    qmpc_solve_kernel<ConvexModel, false, 0>, qmpc_solve_kernel<ConvexModel, false, 1>, qmpc_solve_kernel<ConvexModel, false, 2>,
    qmpc_solve_kernel<Quat8Model, false, 1>,  qmpc_solve_kernel<Quat8Model, false, 2>,
    qmpc_solve_kernel<QuatModel, true, 0>,    qmpc_solve_kernel<QuatModel, true, 1>};
static decltype(&qmpc_ref_kernel<QuatModel, 0>) const kDenseRef[] = {qmpc_ref_kernel<QuatModel, 0>, qmpc_ref_kernel<QuatModel, 1>,
                                                                      qmpc_ref_kernel<ConvexModel, 0>, qmpc_ref_kernel<ConvexModel, 1>,
                                                                      qmpc_ref_kernel<Quat8Model, 1>};
static decltype(&qmpc_linearize_kernel<QuatModel>) const kLinearize[] = {qmpc_linearize_kernel<QuatModel>, qmpc_linearize_kernel<ConvexModel>};
static_assert(sizeof kDenseSolve / sizeof kDenseSolve[0] == kDenseSolveSlots && sizeof kDenseRef / sizeof kDenseRef[0] == kDenseRefSlots &&
                  sizeof kLinearize / sizeof kLinearize[0] == kLinearizeSlots,
              "qmpc_kernel_slots.h");

// qmpc_loop_fused.hip (second translation unit): the closed loop's persistent kernel and the warm-started solve
hipError_t qmpc_loop_fused_set_lds();
hipError_t qmpc_fused_launch(int var, int reference_mode, int convex, int batch, size_t lds, hipStream_t s, const void* dev_params, size_t dev_params_size,
                             const qmpc_loop_params* lp, qmpc_loop_state* st, qmpc_input* rec, double* forces,
                             qmpc_info* info, double* trace_f, double* trace_c, int ticks, double* gws,
                             const qmpc_leg_geometry* geom, double* joint_pos, qmpc_joint_command* cmd,
                             qmpc_joint_command* trace_cmd);
hipError_t qmpc_warm_launch(int var, int convex, int batch, size_t lds, hipStream_t s, const void* dev_params, size_t dev_params_size,
                            const qmpc_input* in, const double* u_init, double* forces, qmpc_info* info, double* traj_u,
                            double* gws, int check_prev);

// qmpc_wform.hip (fourth translation unit): the wave-per-instance kernel with the wrench-form elimination (small batches)
size_t qmpc_wform_slice_doubles(int N, int nl);
hipError_t qmpc_wform_set_lds();
hipError_t qmpc_wform_launch(int model, int ref, int var, int prof, int batch, size_t lds, hipStream_t s, const void* dev_params,
                             size_t dev_params_size, const qmpc_input* in, double* forces, qmpc_info* info, double* traj_u,
                             double* traj_x, long long* prof_out, double* gws);
hipError_t qmpc_wform_launch_list(int var, int grid, size_t lds, hipStream_t s, const void* dev_params, size_t dev_params_size,
                                  const qmpc_input* in, double* forces, qmpc_info* info, double* traj_u, double* traj_x,
                                  const int* sel, const int* sel_count, double* gws, const double* hstate, int hcap);
hipError_t qmpc_wform_inst_expand_launch(int batch, hipStream_t s, const void* dev_params, size_t dev_params_size,
                                         const qmpc_instance_params* rec, void* dev_out, int* status_out);
hipError_t qmpc_wform_inst_solve_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks, const int* status,
                                        const qmpc_input* in, double* forces, qmpc_info* info, double* traj_u, double* traj_x,
                                        double* gws);

// qmpc_loop_inst.hip, qmpc_loop_outcome.hip, qmpc_loop_push.hip, qmpc_loop_ground.hip: the closed loop with per-robot records --
// controller and plant records (qmpc_loop_run_instances*), with the outcome step (qmpc_loop_run_outcomes*), under timed push
// windows (qmpc_loop_run_pushes*), on the robot's true ground (qmpc_loop_run_ground*).  Each unit defines the same entry points in
// its namespace (qmpc_loop_rec.inc): each takes the call's buffers and its records (qmpc_loop_records.h) and passes its kernels what
// they take; the push and ground units have no front kernel of their own.  qmpc_loop_act.hip: the ground loop behind the robot's
// delay line and actuator lag (qmpc_loop_run_actuation*), the same entry points once more, no front kernel either.
// qmpc_loop_sense.hip: the actuation loop whose controller reads a measured state (qmpc_loop_run_sensing*), with a front kernel of
// its own that takes the sensing records.  qmpc_loop_gait.hip: the sensing loop in which every robot walks a gait of its own
// (qmpc_loop_run_gaits*); its front kernel takes the gait record too.  qmpc_loop_motor.hip: the gait loop whose delivered foot force
// respects the motors' torque limits (qmpc_loop_run_motors*); its post and persistent kernels take the geometry and the motor records.
#define QMPC_REC_DECLARE(ns)                                                                                                  \
  namespace ns {                                                                                                               \
  hipError_t rec_set_lds();                                                                                                    \
  hipError_t rec_fused_launch(int var, size_t lds, int ticks, double* gws, const rec_launch& L, const loop_recs& r);           \
  hipError_t rec_front_launch(const rec_launch& L, const loop_recs& r);                                                        \
  hipError_t rec_post_launch(const rec_launch& L, const loop_recs& r);                                                         \
  }
QMPC_REC_DECLARE(qmpc_inst_tu)
QMPC_REC_DECLARE(qmpc_outc_tu)
QMPC_REC_DECLARE(qmpc_push_tu)
QMPC_REC_DECLARE(qmpc_crec_tu)      // qmpc_loop_crec.hip: the three kinds on a ConvexMpc handle (qmpc_set_convex_records)
QMPC_REC_DECLARE(qmpc_ground_tu)    // qmpc_loop_ground.hip
QMPC_REC_DECLARE(qmpc_cground_tu)   // qmpc_loop_cground.hip: the ground call on such a ConvexMpc handle
QMPC_REC_DECLARE(qmpc_act_tu)       // qmpc_loop_act.hip
QMPC_REC_DECLARE(qmpc_cact_tu)      // qmpc_loop_cact.hip: the actuation call on such a ConvexMpc handle
QMPC_REC_DECLARE(qmpc_sense_tu)     // qmpc_loop_sense.hip
QMPC_REC_DECLARE(qmpc_csense_tu)    // qmpc_loop_csense.hip: the sensing call on such a ConvexMpc handle
QMPC_REC_DECLARE(qmpc_gait_tu)      // qmpc_loop_gait.hip
QMPC_REC_DECLARE(qmpc_cgait_tu)     // qmpc_loop_cgait.hip: the gait call on such a ConvexMpc handle
QMPC_REC_DECLARE(qmpc_motor_tu)     // qmpc_loop_motor.hip
QMPC_REC_DECLARE(qmpc_cmotor_tu)    // qmpc_loop_cmotor.hip: the motor call on such a ConvexMpc handle
#undef QMPC_REC_DECLARE
// the launchers of a call with records by [kind][the handle is ConvexMpc's] (REC_*: qmpc_loop_records.h).  QMPC_REC_UNIT(u, f): unit
// u's, with the front kernel of unit f (the QuatMpc units of REC_PUSH .. REC_ACT launch the outcome unit's); one ConvexMpc unit
// serves the first three kinds
#define QMPC_REC_UNIT(u, f) {u::rec_set_lds, u::rec_fused_launch, f::rec_front_launch, u::rec_post_launch}
static const struct {
  decltype(&qmpc_inst_tu::rec_set_lds) set_lds;
  decltype(&qmpc_inst_tu::rec_fused_launch) fused_launch;
  decltype(&qmpc_inst_tu::rec_front_launch) front_launch;
  decltype(&qmpc_inst_tu::rec_post_launch) post_launch;
} kRec[REC_KINDS][2] = {{QMPC_REC_UNIT(qmpc_inst_tu, qmpc_inst_tu), QMPC_REC_UNIT(qmpc_crec_tu, qmpc_crec_tu)},
                        {QMPC_REC_UNIT(qmpc_outc_tu, qmpc_outc_tu), QMPC_REC_UNIT(qmpc_crec_tu, qmpc_crec_tu)},
                        {QMPC_REC_UNIT(qmpc_push_tu, qmpc_outc_tu), QMPC_REC_UNIT(qmpc_crec_tu, qmpc_crec_tu)},
                        {QMPC_REC_UNIT(qmpc_ground_tu, qmpc_outc_tu), QMPC_REC_UNIT(qmpc_cground_tu, qmpc_cground_tu)},
                        {QMPC_REC_UNIT(qmpc_act_tu, qmpc_outc_tu), QMPC_REC_UNIT(qmpc_cact_tu, qmpc_cact_tu)},
                        {QMPC_REC_UNIT(qmpc_sense_tu, qmpc_sense_tu), QMPC_REC_UNIT(qmpc_csense_tu, qmpc_csense_tu)},
                        {QMPC_REC_UNIT(qmpc_gait_tu, qmpc_gait_tu), QMPC_REC_UNIT(qmpc_cgait_tu, qmpc_cgait_tu)},
                        {QMPC_REC_UNIT(qmpc_motor_tu, qmpc_motor_tu), QMPC_REC_UNIT(qmpc_cmotor_tu, qmpc_cmotor_tu)}};
#undef QMPC_REC_UNIT
// ... and the kernels each unit has beside them: the expansions of the plant blocks and the check of the windows
hipError_t qmpc_loop_inst_expand_launch(hipStream_t s, const void* dev_params, size_t dev_params_size, const qmpc_plant_params* plant,
                                        const qmpc_instance_params* ctrl, const int* ctrl_status, void* bcast_out, void* plants_out,
                                        int batch);
hipError_t qmpc_loop_outcome_expand_base_launch(hipStream_t s, const void* dev_params, size_t dev_params_size, void* bcast_out,
                                                void* plants_out, int batch);
hipError_t qmpc_loop_push_check_launch(hipStream_t s, const qmpc_push_params* push, int per_robot, void* plants, int batch);
namespace qmpc_ground_tu {
hipError_t rec_ground_check_launch(hipStream_t s, const qmpc_ground_params* ground, void* plants, int batch);
}
namespace qmpc_act_tu {
hipError_t rec_act_check_launch(hipStream_t s, const qmpc_actuation_params* act, const qmpc_actuation_line* line, void* plants, int batch);
}
namespace qmpc_sense_tu {
hipError_t rec_sense_check_launch(hipStream_t s, const qmpc_sense_params* sense, void* plants, int batch);
}
namespace qmpc_gait_tu {
hipError_t rec_gait_check_launch(hipStream_t s, const qmpc_gait_params* gait, void* plants, double dt, int batch);
}
namespace qmpc_motor_tu {
hipError_t rec_motor_check_launch(hipStream_t s, const qmpc_motor_params* motor, const qmpc_motor_tally* mtally, void* plants, int batch);
}

// qmpc_lane.hip (third translation unit): the lane-per-instance kernel of large batches
size_t qmpc_lane_ws_bytes(int N, int nl, unsigned slots, int wide);
size_t qmpc_lane_scratch_bytes(int batch);
int qmpc_lane_param_slots();
hipError_t qmpc_lane_upload_params(int pslot, hipStream_t s, const void* dev_params, size_t dev_params_size);
hipError_t qmpc_lane_launch(int nl, int pslot, int batch, hipStream_t s, const void* dev_params, size_t dev_params_size, const void* in,
                            double* forces, qmpc_info* info, double* ws, unsigned slots, int* scratch, int upload_params,
                            const double* u_init, double* traj_u, int check_prev, int order_prev, double* traj_x, int iter_cap,
                            int* hcount, int* hsel, double* hstate, int hcap, int pair);
size_t qmpc_lane_handoff_list_bytes(int batch);
size_t qmpc_lane_handoff_record_doubles(int N);
hipError_t qmpc_lane_sort_launch(int batch, hipStream_t s, const void* in, int* scratch);

// qmpc_lane_inst.hip, qmpc_lane_inst_warm.hip, qmpc_lane_cinst.hip, qmpc_lane_cinst_warm.hip: per-instance parameters on the lane
// kernel (QMPC_INSTANCES_AUTO; ConvexMpc: qmpc_set_convex_lane_records) -- cold and warm-started, QuatMpc's and ConvexMpc's.  Each
// unit defines the same two entry points (qmpc_lane_inst_kernel.inc) and ignores the trailing arguments its kernel does not take;
// the cold units also define the sort of their model's ticks.
size_t qmpc_lane_inst_param_bytes(unsigned slots);
#define QMPC_LANE_INST_DECLARE(name)                                                                                                  \
  hipError_t name##_upload_params(int pslot, hipStream_t s, const void* dev_params, size_t dev_params_size);                         \
  hipError_t name##_launch_only(int pslot, int batch, hipStream_t s, const void* in, const void* dev_blocks, const int* status,      \
                                double* forces, qmpc_info* info, double* ws, double* prm, unsigned slots, const int* perm,           \
                                const double* u_init, double* traj_u, double* traj_x, int check_prev, int iter_cap, int* hcount,     \
                                int* hsel, double* hstate, int hcap, int pair);
#define QMPC_LANE_INST_DECLARE_SORT(name)                                                                                             \
  hipError_t name##_sort_launch(int batch, hipStream_t s, const void* in, const qmpc_info* prev, const int* status, int idle_last,   \
                                int* scratch);
QMPC_LANE_INST_DECLARE(qmpc_lane_inst)
QMPC_LANE_INST_DECLARE(qmpc_lane_inst_warm)
QMPC_LANE_INST_DECLARE(qmpc_lane_cinst)
QMPC_LANE_INST_DECLARE(qmpc_lane_cinst_warm)
QMPC_LANE_INST_DECLARE_SORT(qmpc_lane_inst)
QMPC_LANE_INST_DECLARE_SORT(qmpc_lane_cinst)
#undef QMPC_LANE_INST_DECLARE
#undef QMPC_LANE_INST_DECLARE_SORT
static const struct {
  decltype(&qmpc_lane_inst_sort_launch) sort_launch;      // the model's idle-last sort
  struct {
    decltype(&qmpc_lane_inst_upload_params) upload_params;
    decltype(&qmpc_lane_inst_launch_only) launch_only;
  } start[2];
} kLaneInst[2] = {      // [convex].start[warm]
    {qmpc_lane_inst_sort_launch,
     {{qmpc_lane_inst_upload_params, qmpc_lane_inst_launch_only}, {qmpc_lane_inst_warm_upload_params, qmpc_lane_inst_warm_launch_only}}},
    {qmpc_lane_cinst_sort_launch,
     {{qmpc_lane_cinst_upload_params, qmpc_lane_cinst_launch_only}, {qmpc_lane_cinst_warm_upload_params, qmpc_lane_cinst_warm_launch_only}}}};
// qmpc_wform_inst_list.hip: the lane kernel's hand-off with per-instance parameters
hipError_t qmpc_wform_inst_list_set_lds();
hipError_t qmpc_wform_inst_list_launch(int var, int grid, size_t lds, hipStream_t s, const void* dev_blocks, const qmpc_input* in,
                                       double* forces, qmpc_info* info, double* traj_u, double* traj_x, const int* sel,
                                       const int* sel_count, double* gws, const double* hstate, int hcap);
// qmpc_wform_inst_warm.hip, qmpc_wform_cinst_warm.hip: the warm-started ticks of a closed loop with controller records on the wave
// kernels (qmpc_set_loop_warm_records; ConvexMpc: qmpc_set_convex_warm_records)
hipError_t qmpc_wform_inst_warm_set_lds();
hipError_t qmpc_loop_row_reset_launch(hipStream_t s, int* row);
hipError_t qmpc_wform_inst_warm_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks, const int* status,
                                       const qmpc_input* in, const double* u_init, double* forces, qmpc_info* info, double* traj_u,
                                       double* gws, int check_prev);
hipError_t qmpc_wform_cinst_warm_set_lds();
hipError_t qmpc_wform_cinst_warm_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks, const int* status,
                                        const qmpc_input* in, const double* u_init, double* forces, qmpc_info* info, double* traj_u,
                                        double* gws, int check_prev);

// qmpc_wform_sched.hip: QuatMpc's solve with a contact schedule over the horizon (qmpc_solve_schedule*)
hipError_t qmpc_wform_sched_set_lds();
hipError_t qmpc_wform_sched_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks, const int* status,
                                   const qmpc_input* in, const unsigned char* sched, double* forces, qmpc_info* info, double* traj_u,
                                   double* traj_x, double* gws);
hipError_t qmpc_wform_sched_expand_uniform_launch(int batch, hipStream_t s, const void* dev_params, size_t dev_params_size,
                                                  const qmpc_instance_params* rec, void* dev_out, int* status_out);

// qmpc_wform_cinst.hip: ConvexMpc's solve with per-instance parameters (qmpc_convex_solve_instances*)
hipError_t qmpc_wform_cinst_set_lds();
hipError_t qmpc_wform_cinst_solve_launch(int var, int batch, size_t lds, hipStream_t s, const void* dev_blocks, const int* status,
                                         const qmpc_input* in, double* forces, qmpc_info* info, double* traj_u, double* traj_x,
                                         double* gws);

struct qmpc_handle {
  qmpc_params params;
  DevParams dev;
  qmpc_select sel;        // what the choice of kernel depends on, and the tuning knobs (qmpc_plan.h)
  int device;
  int max_batch;
  hipStream_t stream;
  hipEvent_t ev0, ev1;
  bool timed;
  qmpc_input* d_in;
  double* d_forces;
  qmpc_info* d_info;
  double* d_traj_u;
  double* d_traj_x;
  double* d_A;
  double* d_B;
  int* d_loop_row;        // trace row counter of the closed loop (qmpc_loop_run*)
  double* d_leg;          // staging of the host-buffer leg calls (grown on demand, freed with the handle)
  size_t leg_cap;         // its capacity in doubles
  double* d_loop;         // staging of qmpc_loop_run (states and traces; grown on demand, freed with the handle)
  size_t loop_cap;        // its capacity in doubles
  double* d_gws;          // [max_batch][N*(156+84)] workspace of the global-gains variant
  double* d_lane_ws;      // structure-of-arrays workspace of the lane-per-instance kernel: [elements][lane_slots], on first use
  unsigned lane_slots;    // resident lanes it is sized for
  int* d_lane_scratch;    // counting sort of the batch on the stance mask: hist | cursor | perm[max_batch]
  int lane_pslot;         // this handle's slot in the lane kernel's constant-memory parameter table (-1: none)
  int* d_handoff;              // straggler hand-off: count | list of instances the capped lane launch left (on first use)
  double* d_hstate;            // ... and their state records (hstate_cap of them)
  int hstate_cap;
  qmpc_opts opts;              // the run-time settings the planners of the calls with records read (qmpc_plan.h): the policy of
                               // qmpc_set_instances_policy (default WAVE), handoff_failed (the hand-off records could not be allocated --
                               // this handle runs the pure lane kernel, qmpc_query), the opt-ins of qmpc_set_loop_warm_records (the loops
                               // with controller records accept lp->warm_start; ConvexMpc: qmpc_set_convex_warm_records) and
                               // qmpc_set_convex_records (the loops with records accept this ConvexMpc handle; then d_outcome is also the scratch the outcome step of a call without outcome
                               // records runs on)
  int last_kernel;             // QMPC_KERNEL_* of the most recent solve launch (qmpc_query)
  // host-buffer calls (qmpc_solve*, qmpc_solve_async): pinned staging owned by the handle.  Batches below the lane kernel's
  // threshold are solved ZERO-COPY: the wavefront of an instance reads its 384-byte record from pinned host memory with its
  // one coalesced load and writes forces / status straight back, so H2D, kernel and D2H are one launch and one
  // synchronisation (records cross the link while other wavefronts compute)
  unsigned char* h_stage_in;   // [max_batch] records
  unsigned char* h_stage_out;  // [max_batch] (forces | info)
  int zero_copy;               // env QMPC_ZERO_COPY (default 1); 0 as well when no pinned memory is to be had
  struct { double* forces; qmpc_info* info; size_t fbytes, ibytes; } pending;   // copy-out owed to a pageable caller (qmpc_wait)
  int stage_in_busy;           // a non-blocking zero-copy launch may still be READING its records from h_stage_in: the staging is
                               // not refilled before the stream has drained (qmpc_solve_async with a pageable `in`, pinned outputs)
  unsigned char* d_inst;       // per-instance parameters (qmpc_solve_instances*), on first use: [max_batch] DevParams | [max_batch]
                               // qmpc_instance_params (staging of the host-buffer call) | [max_batch] int verdicts
  double* d_lane_prm;          // ... under QMPC_INSTANCES_AUTO: the resident wavefronts' parameter blocks [LPR_ROWS][lane_slots], on first use
  unsigned char* d_plant;      // per-robot plants of qmpc_loop_run_instances*, on first use: [max_batch] PlantDev | [max_batch]
                               // qmpc_plant_params (staging of the host-buffer call)
  qmpc_loop_outcome* d_outcome;   // staging of qmpc_loop_run_outcomes (the host-buffer call), on its first use: [max_batch] records
  qmpc_push_params* d_push;       // staging of qmpc_loop_run_pushes (the host-buffer call), on its first use: [max_batch][push_cap]
  int push_cap;                   // ... windows per robot it holds (grown when a call brings more)
  // staging of the optional record kinds of the host-buffer calls (qmpc_loop_run_ground .. qmpc_loop_run_motors), each on its
  // first use: which records a buffer holds, in which order and at which size is kRecStage's to say (below, at loop_records_host)
  void* d_ground;
  void* d_act;
  void* d_sense;
  void* d_gait;
  void* d_motor;
  unsigned char* d_sched;         // staging of qmpc_solve_schedule (the host-buffer call), on its first use: max_batch schedules
                                  // of N bytes
};

// The staging of the optional record kinds of a host-buffer call, one row per record in the order of the copies in (the copies
// out walk the rows backwards): the handle's buffer, the record's size, the size of the record that lies BEFORE it in the buffer
// (a buffer is max_batch records of one type, then max_batch of the other; 0: this one comes first), whether the record comes
// back, and the record's place in loop_recs.  Allocation (loop_records_host), both copies and qmpc_query's byte count walk it.
struct rec_stage {
  void* qmpc_handle::*buf;
  size_t elem, before;
  bool out;
  void* (*get)(const loop_recs&);
  void (*set)(loop_recs&, void*);
};
#define QMPC_STAGE(buf_, T_, before_, out_, field_)                                                                   \
  {&qmpc_handle::buf_, sizeof(T_), before_, out_,                                                                     \
   [](const loop_recs& r) -> void* { return const_cast<void*>(static_cast<const void*>(r.field_)); },                 \
   [](loop_recs& r, void* p) { r.field_ = static_cast<T_*>(p); }}
static const rec_stage kRecStage[] = {QMPC_STAGE(d_ground, qmpc_ground_params, 0, false, ground),
                                      QMPC_STAGE(d_ground, qmpc_ground_tally, sizeof(qmpc_ground_params), true, tally),
                                      QMPC_STAGE(d_act, qmpc_actuation_params, sizeof(qmpc_actuation_line), false, act),
                                      QMPC_STAGE(d_act, qmpc_actuation_line, 0, true, line),
                                      QMPC_STAGE(d_sense, qmpc_sense_params, 0, false, sense),
                                      QMPC_STAGE(d_sense, qmpc_sense_seen, sizeof(qmpc_sense_params), true, seen),
                                      QMPC_STAGE(d_gait, qmpc_gait_params, 0, false, gait),
                                      QMPC_STAGE(d_motor, qmpc_motor_params, sizeof(qmpc_motor_tally), false, motor),
                                      QMPC_STAGE(d_motor, qmpc_motor_tally, 0, true, mtally)};
#undef QMPC_STAGE

constexpr unsigned kLaneMaxSlots = 1024 * 64;   // one wavefront per SIMD of the chip

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      std::fprintf(stderr, "qmpc: %s failed: %s\n", #expr, hipGetErrorString(e_));         \
      return QMPC_HIP_ERROR;                                                               \
    }                                                                                      \
  } while (0)

extern "C" {

const char* qmpc_version(void) { return "qmpc-hip 0.3 (gfx950, wave-per-instance IPM/Riccati with fp64 MFMA; lane-per-instance kernel for large batches; device-resident closed loop)"; }
int32_t qmpc_sizeof_input(void) { return (int32_t)sizeof(qmpc_input); }
int32_t qmpc_sizeof_params(void) { return (int32_t)sizeof(qmpc_params); }
int32_t qmpc_sizeof_info(void) { return (int32_t)sizeof(qmpc_info); }
int32_t qmpc_sizeof_convex_input(void) { return (int32_t)sizeof(qmpc_convex_input); }
int32_t qmpc_sizeof_input8(void) { return (int32_t)sizeof(qmpc_input8); }
static_assert(sizeof(qmpc_input8) == 8 * Dim<8>::REC && sizeof(qmpc_input) == 8 * Dim<4>::REC, "record sizes");
// free list of the lane kernel's parameter slots (qmpc_lane.hip: ql_params[])
static std::mutex g_lane_slot_mutex;
static unsigned long long g_lane_slot_used = 0;
static int lane_slot_acquire() {
  std::lock_guard<std::mutex> lock(g_lane_slot_mutex);
  const int n = qmpc_lane_param_slots();
  for (int i = 0; i < n && i < 64; ++i)
    if (!((g_lane_slot_used >> i) & 1ull)) { g_lane_slot_used |= 1ull << i; return i; }
  return -1;
}
static void lane_slot_release(int slot) {
  if (slot < 0) return;
  std::lock_guard<std::mutex> lock(g_lane_slot_mutex);
  g_lane_slot_used &= ~(1ull << slot);
}
static_assert(sizeof(qmpc_convex_input) == sizeof(qmpc_input), "both records are 48 doubles");

const char* qmpc_status_string(int32_t s) {
  switch (s) {
    case QMPC_OK: return "ok";
    case QMPC_MAX_ITER: return "iteration cap reached";
    case QMPC_NO_CONTACT: return "no stance leg";
    case QMPC_NAN_INPUT: return "non-finite input";
    case QMPC_LINESEARCH_FAIL: return "line search failed";
    case QMPC_NOT_PD: return "Quu not positive definite";
    case QMPC_BAD_PARAMS: return "invalid per-instance parameters";
    case QMPC_BAD_ARGUMENT: return "bad argument";
    case QMPC_NO_DEVICE: return "no HIP device (there is no CPU fallback)";
    case QMPC_HIP_ERROR: return "HIP runtime error";
    case QMPC_BATCH_TOO_LARGE: return "batch exceeds the handle's capacity";
    case QMPC_UNSUPPORTED: return "optional dependency not available";
    default: return "unknown status";
  }
}

// legged_ctrl/config/gazebo_go1_quat_mpc.yaml:36-75,115-122; QuatMpc.cpp:21-26,182
void qmpc_default_params(qmpc_params* p, int32_t horizon, int32_t mode) {
  std::memset(p, 0, sizeof *p);
  p->horizon = horizon;
  p->h = (float)(10.0 / 1000.0);
  p->h_ref = 10.0 / 1000.0;
  p->mass = 12.84;
  const double trunk[3] = {0.0168128557, 0.063009565, 0.0716547275};
  for (int a = 0; a < 3; ++a) p->inertia[4 * a] = 1.2 * trunk[a];
  const double q[13] = {2.5, 2.5, 10.0, 0, 0, 0, 0, 0.1, 0.1, 0.1, 0.15, 0.15, 0.15};
  std::memcpy(p->q_weights, q, sizeof q);
  for (int j = 0; j < 12; ++j) p->r_weights[j] = 0.000001;
  p->w = 50.0;
  p->mu = 0.7;
  p->fz_max = 100.0;
  p->mode = mode;
  p->penalty_initial = 1.0;
  p->penalty_max = 1e8;
  p->tol_stationarity = 1e-4;
  p->tol_cost_intermediate = 1e-4;
  p->linesearch_max = 10;
  p->drop_ang_vel = 1;
  if (mode == QMPC_MODE_REFERENCE) {
    p->iterations_max = 10;     // QuatMpc.cpp:22
    p->penalty_scaling = 20.0;  // QuatMpc.cpp:26
    p->tol_feasibility = 1e-4;
  } else {
    p->iterations_max = 120;  // horizon 32 needs up to 86 interior-point iterations on the synthetic states
    p->penalty_scaling = 10.0;
    p->tol_feasibility = 1e-8;
    p->tol_step = 1e-8;
    p->ipm_mu0 = 0.01;
    p->ipm_mu_final = 1e-12;
    p->ipm_sigma = 0.2;
    p->ipm_sigma_fast = 0.01;
    p->ipm_tau = 0.995;
  }
}

// legged_ctrl/config/gazebo_go1_convex_mpc.yaml:35-73; AltroUtils.cpp:239,270-272 (the model's
// hard-coded mass and un-scaled trunk inertia); ConvexMpc.cpp:36-38
void qmpc_default_convex_params(qmpc_params* p, int32_t horizon, int32_t mode) {
  qmpc_default_params(p, horizon, mode);
  p->model = QMPC_MODEL_CONVEX;
  p->h = (float)(5.0 / 1000.0);
  p->h_ref = 5.0 / 1000.0;
  const double trunk[3] = {0.0168128557, 0.063009565, 0.0716547275};
  for (int a = 0; a < 3; ++a) p->inertia[4 * a] = trunk[a];
  const double q[13] = {3.0, 3.0, 3.0, 1.0, 1.0, 20.0, 0.0, 0.0, 3.0, 2.0, 3.0, 2.0, 0.0};
  std::memcpy(p->q_weights, q, sizeof q);
  p->w = 0.0;
  p->mu = 0.6;
  p->fz_max = 200.0;
  p->drop_ang_vel = 0;
  if (mode == QMPC_MODE_REFERENCE) p->iterations_max = 5;   // ConvexMpc.cpp:37
}

// BASELINE.json config 5: SYNTHETIC 30 kg biped, two 0.2 x 0.1 m feet with 4 corner contact points
// each.  The humanoid branch is not in the reference checkout; nothing upstream pins these values.
void qmpc_default_biped8_params(qmpc_params* p, int32_t horizon, int32_t mode) {
  qmpc_default_params(p, horizon, mode);
  p->model = QMPC_MODEL_QUAT8;
  p->mass = 30.0;
  std::memset(p->inertia, 0, sizeof p->inertia);
  p->inertia[0] = 1.2; p->inertia[4] = 1.0; p->inertia[8] = 0.3;
  p->fz_max = 250.0;
}

qmpc_status qmpc_set_params(qmpc_handle* h, const qmpc_params* params) {
  if (!h || !params) return QMPC_BAD_ARGUMENT;
  DevParams d;
  const int st = fill_dev_params(params, &d);
  if (st != QMPC_OK) return (qmpc_status)st;
  if (params->horizon != h->params.horizon) return QMPC_BAD_ARGUMENT;  // buffers are sized by N
  if (params->model != h->params.model) return QMPC_BAD_ARGUMENT;
  h->params = *params;
  h->dev = d;
  h->sel.mode = params->mode;      // (what the choice reads of the parameters)
  h->sel.iterations_max = params->iterations_max;
  return QMPC_OK;
}

// device resources of a handle; on failure the caller destroys the (partially filled) handle
static qmpc_status create_resources(qmpc_handle* h, int N, int nl, int nu) {
  const qmpc_params* params = &h->params;
  const int32_t max_batch = h->max_batch;
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&h->ev0));
  HIP_TRY(hipEventCreate(&h->ev1));
  HIP_TRY(hipMalloc(&h->d_in, sizeof(double) * (32 + 4 * nl) * (size_t)max_batch));
  HIP_TRY(hipMalloc(&h->d_forces, sizeof(double) * nu * (size_t)max_batch));
  HIP_TRY(hipMalloc(&h->d_info, sizeof(qmpc_info) * (size_t)max_batch));
  // the dynamic LDS limit of every wave kernel of the library (qmpc_fill_select has refused the layouts beyond 160 KB)
  HIP_TRY(set_max_lds(kDenseSolve, kDenseRef, kLinearize));
  HIP_TRY(qmpc_loop_fused_set_lds());
  HIP_TRY(qmpc_wform_set_lds());
  for (int k = 0; k < REC_KINDS; ++k)
    for (int c = 0; c < 2; ++c)      // (once per unit: the ConvexMpc unit of the first three kinds is one)
      if (k == 0 || kRec[k][c].set_lds != kRec[k - 1][c].set_lds) HIP_TRY(kRec[k][c].set_lds());
  HIP_TRY(qmpc_wform_inst_list_set_lds());
  HIP_TRY(qmpc_wform_inst_warm_set_lds());
  HIP_TRY(qmpc_wform_cinst_set_lds());
  HIP_TRY(qmpc_wform_cinst_warm_set_lds());
  HIP_TRY(qmpc_wform_sched_set_lds());
  HIP_TRY(hipMalloc(&h->d_gws, sizeof(double) * (size_t)N * (13 * nu + 21 * nl + 30 * nl) * (size_t)max_batch));
  return QMPC_OK;
}

qmpc_status qmpc_create(const qmpc_params* params, int32_t max_batch, int32_t device, qmpc_handle** out) {
  if (!out) return QMPC_BAD_ARGUMENT;
  *out = nullptr;
  if (!params || max_batch < 1) return QMPC_BAD_ARGUMENT;
  DevParams d;
  const int st = fill_dev_params(params, &d);
  if (st != QMPC_OK) return (qmpc_status)st;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) {
    std::fprintf(stderr, "qmpc_create: no HIP device %d (found %d); there is no CPU fallback\n", device, ndev);
    return QMPC_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  qmpc_handle* h = new (std::nothrow) qmpc_handle();
  if (!h) return QMPC_HIP_ERROR;
  std::memset(h, 0, sizeof *h);
  h->opts = qmpc_opts();
  h->params = *params;
  h->dev = d;
  h->device = device;
  h->max_batch = max_batch;
  const int N = params->horizon;
  const int nl = model_nl(params->model), nu = 3 * nl;
  // the lane kernel reads its parameters from a constant-memory table with one slot per LIVE handle (a slot is rewritten
  // before every launch of its handle, on that launch's stream): slots come from a free list and go back in
  // qmpc_destroy; a handle created while all of them are taken keeps the wave-per-instance kernels
  h->lane_pslot = lane_slot_acquire();
  if (!qmpc_fill_select(&h->sel, params, std::getenv, h->lane_pslot >= 0)) {
    lane_slot_release(h->lane_pslot);
    delete h;
    return QMPC_BAD_ARGUMENT;
  }
  h->zero_copy = h->sel.zero_copy;
  const qmpc_status rs = create_resources(h, N, nl, nu);
  if (rs != QMPC_OK) { qmpc_destroy(h); return rs; }   // release whatever was created
  *out = h;
  return QMPC_OK;
}

void qmpc_destroy(qmpc_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->d_in) (void)hipFree(h->d_in);
  if (h->d_forces) (void)hipFree(h->d_forces);
  if (h->d_gws) (void)hipFree(h->d_gws);
  if (h->d_lane_ws) (void)hipFree(h->d_lane_ws);
  if (h->d_lane_scratch) (void)hipFree(h->d_lane_scratch);
  if (h->d_handoff) (void)hipFree(h->d_handoff);
  if (h->d_hstate) (void)hipFree(h->d_hstate);
  if (h->h_stage_in) (void)hipHostFree(h->h_stage_in);
  if (h->h_stage_out) (void)hipHostFree(h->h_stage_out);
  if (h->d_leg) (void)hipFree(h->d_leg);
  if (h->d_loop_row) (void)hipFree(h->d_loop_row);
  if (h->d_loop) (void)hipFree(h->d_loop);
  if (h->d_info) (void)hipFree(h->d_info);
  if (h->d_traj_u) (void)hipFree(h->d_traj_u);
  if (h->d_traj_x) (void)hipFree(h->d_traj_x);
  if (h->d_A) (void)hipFree(h->d_A);
  if (h->d_B) (void)hipFree(h->d_B);
  if (h->d_inst) (void)hipFree(h->d_inst);
  if (h->d_lane_prm) (void)hipFree(h->d_lane_prm);
  if (h->d_plant) (void)hipFree(h->d_plant);
  if (h->d_outcome) (void)hipFree(h->d_outcome);
  if (h->d_push) (void)hipFree(h->d_push);
  if (h->d_ground) (void)hipFree(h->d_ground);
  if (h->d_act) (void)hipFree(h->d_act);
  if (h->d_sense) (void)hipFree(h->d_sense);
  if (h->d_gait) (void)hipFree(h->d_gait);
  if (h->d_motor) (void)hipFree(h->d_motor);
  if (h->d_sched) (void)hipFree(h->d_sched);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  lane_slot_release(h->lane_pslot);      // after the frees above (they wait for the device): no launch of this handle reads the slot any more
  delete h;
}


// workspace of the lane kernel, allocated at first use (never inside a stream capture: qmpc_loop_run calls this first)
static qmpc_status ensure_lane_buffers(qmpc_handle* h) {
  const int nl = model_nl(h->params.model);
  if (!h->d_lane_ws) {
    // one workspace block per wavefront; a wavefront may run with 32 of its lanes (qmpc_lane.hip), hence max_batch / 32
    const unsigned want = (unsigned)(((size_t)h->max_batch + 31) / 32) * 64;
    h->lane_slots = want < kLaneMaxSlots ? want : kLaneMaxSlots;
    // both buffers or none: a handle with a workspace but no sort scratch would run unsorted for the rest of its life
    double* ws = nullptr;
    int* sc = nullptr;
    if (hipMalloc(&ws, qmpc_lane_ws_bytes(h->params.horizon, nl, h->lane_slots, h->params.mode == QMPC_MODE_REFERENCE)) != hipSuccess ||
        hipMalloc(&sc, qmpc_lane_scratch_bytes(h->max_batch)) != hipSuccess) {
      std::fprintf(stderr, "qmpc: lane-kernel workspace allocation failed: %s\n", hipGetErrorString(hipGetLastError()));
      if (ws) (void)hipFree(ws);
      return QMPC_HIP_ERROR;
    }
    h->d_lane_ws = ws;
    h->d_lane_scratch = sc;
  }
  return QMPC_OK;
}
// Hand-off buffers, on first use.  One state record (8 + 84 N doubles) per instance of the handle's capacity: 8-10 % of a batch
// is handed over in the measured workloads, but WHICH record an instance gets is decided by an atomic counter, so only room
// for all of them keeps the results independent of timing (445 MB at 65536 x N=10, 1.8 GB at 262144 x N=10; held until
// qmpc_destroy, like the lane kernel's workspace).  If the memory is not there the hand-off is switched off for this handle.
static bool ensure_handoff_buffers(qmpc_handle* h) {
  if (h->d_handoff) return true;
  if (h->opts.handoff_failed) return false;
  h->hstate_cap = h->max_batch;
  const size_t rec_bytes = sizeof(double) * qmpc_lane_handoff_record_doubles(h->params.horizon);
  if (hipMalloc(&h->d_handoff, qmpc_lane_handoff_list_bytes(h->max_batch)) != hipSuccess ||
      hipMalloc(&h->d_hstate, rec_bytes * (size_t)h->hstate_cap) != hipSuccess) {
    // NOT silent: a handle without records runs the pure lane kernel, whose results agree with the hand-off's to ~1e-10 N but
    // not bit for bit -- the caller can see it (stderr, qmpc_query(QMPC_QUERY_HANDOFF_ACTIVE)) and avoid it (qmpc_prepare
    // right after qmpc_create, before other allocations take the memory)
    std::fprintf(stderr, "qmpc: straggler hand-off records (%zu MB) could not be allocated: %s -- this handle keeps the pure lane kernel\n",
                 (rec_bytes * (size_t)h->hstate_cap) >> 20, hipGetErrorString(hipGetLastError()));
    if (h->d_handoff) (void)hipFree(h->d_handoff);
    h->d_handoff = nullptr; h->d_hstate = nullptr;
    h->opts.handoff_failed = true;
    return false;
  }
  return true;
}
// The lane kernel as `p` plans it (its buffers allocated already), and the hand-off's list kernel after it where the plan caps it.
// d_u_init / d_traj_u: previous solutions [batch][N][3 NL] to start from (null: cold) / where to leave this one (null:
// not wanted); they may be the same buffer.  check_prev: d_info still holds the records of the previous solves.
// restart (QMPC_HANDOFF_RESTART, plain solves): the list kernel ignores the state records and solves from scratch
static qmpc_status launch_lane(qmpc_handle* h, const qmpc_plan& p, int32_t batch, const qmpc_input* d_in, double* d_forces,
                               qmpc_info* d_info, hipStream_t s, const double* d_u_init, double* d_traj_u, int check_prev,
                               double* d_traj_x, bool restart) {
  const int nl = h->params.model == QMPC_MODEL_CONVEX ? -4 : model_nl(h->params.model);     // -4: ConvexMpc's model (qmpc_lane.hip)
  const bool cap = p.iter_cap > 0;
  HIP_TRY(qmpc_lane_launch(nl, h->lane_pslot, (int)batch, s, &h->dev, sizeof h->dev, d_in, d_forces, d_info, h->d_lane_ws, h->lane_slots,
                           h->sel.lane_sort ? h->d_lane_scratch : nullptr, p.upload_params, d_u_init, d_traj_u, check_prev, p.order_prev,
                           d_traj_x, p.iter_cap, cap ? h->d_handoff : nullptr, cap ? h->d_handoff + 64 : nullptr, cap ? h->d_hstate : nullptr,
                           h->hstate_cap, h->sel.lane_pair));
  if (cap)      // one workgroup per SIMD walks the list the lane kernel left (8-10 % of the batch in the measured workloads)
    HIP_TRY(qmpc_wform_launch_list(p.handoff_variant, p.handoff_grid, p.lds, s, &h->dev, sizeof h->dev, d_in, d_forces, d_info, d_traj_u,
                                   d_traj_x, h->d_handoff + 64, h->d_handoff, p.gws ? h->d_gws : nullptr, restart ? nullptr : h->d_hstate,
                                   h->hstate_cap));
  return QMPC_OK;
}

// a plain solve (kind PLAIN) or a tick of the cold-started closed loop (LOOP_TICK: not timed; its lane kernel's buffers and
// parameters are set up before the loop captures its ticks)
static qmpc_status launch_solve(qmpc_handle* h, int32_t batch, const qmpc_input* d_in, double* d_forces,
                                qmpc_info* d_info, double* d_tu, double* d_tx, hipStream_t s, qmpc_call kind = QMPC_CALL_PLAIN) {
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;   // the gains workspace is sized by max_batch
  const bool timed = kind == QMPC_CALL_PLAIN;
  if (timed) HIP_TRY(hipEventRecord(h->ev0, s));
  qmpc_plan p = plan(h->sel, batch, kind, d_info != nullptr, h->opts.handoff_failed);
  const bool ref = h->params.mode == QMPC_MODE_REFERENCE;
  double* gws = p.gws ? h->d_gws : nullptr;
  if (p.variant == 4) {
    const qmpc_status es = ensure_lane_buffers(h);
    if (es != QMPC_OK) return es;
    // (the hand-off records are allocated on first use; without them the pure lane kernel)
    if (p.iter_cap && !ensure_handoff_buffers(h)) p = plan(h->sel, batch, kind, true, h->opts.handoff_failed);
    const qmpc_status ls = launch_lane(h, p, batch, d_in, d_forces, d_info, s, nullptr, d_tu, 0, d_tx, h->sel.handoff_restart);
    if (ls != QMPC_OK) return ls;
  } else if (p.variant >= 3) {      // the wrench-form kernels (qmpc_wform.hip)
    HIP_TRY(qmpc_wform_launch(h->params.model, ref, p.variant, 0, (int)batch, p.lds, s, &h->dev, sizeof h->dev, d_in, d_forces, d_info, d_tu,
                              d_tx, nullptr, gws));
  } else {      // the round-1 kernels; the reference's own AL-iLQR mode on them: qmpc_ref.hip
    const int model = h->params.model;
    const int k = ref ? dense_ref_slot(model, p.variant) : dense_solve_slot(model, p.variant, false);
    if (k < 0) HIP_TRY(hipErrorInvalidValue);
    if (ref)
      hipLaunchKernelGGL(kDenseRef[k], dim3((unsigned)batch), dim3(kWave), p.lds, s, h->dev, d_in, d_forces, d_info, d_tu, d_tx, (int)batch, gws);
    else
      hipLaunchKernelGGL(kDenseSolve[k], dim3((unsigned)batch), dim3(kWave), p.lds, s, h->dev, d_in, d_forces, d_info, d_tu, d_tx, (int)batch,
                         (long long*)nullptr, gws);
    HIP_TRY(hipGetLastError());
  }
  h->last_kernel = p.family;
  if (timed) {
    HIP_TRY(hipEventRecord(h->ev1, s));
    h->timed = true;
  }
  return QMPC_OK;
}

qmpc_status qmpc_solve_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in, double* d_forces_body,
                              qmpc_info* d_info, void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_in || !d_forces_body))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != QMPC_MODEL_QUAT) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  return launch_solve(h, batch, d_in, d_forces_body, d_info, nullptr, nullptr, s);
}

qmpc_status qmpc_solve8_device(qmpc_handle* h, int32_t batch, const qmpc_input8* d_in, double* d_forces_body,
                               qmpc_info* d_info, void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_in || !d_forces_body))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != QMPC_MODEL_QUAT8) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  return launch_solve(h, batch, reinterpret_cast<const qmpc_input*>(d_in), d_forces_body, d_info, nullptr, nullptr, s);
}

qmpc_status qmpc_convex_solve_device(qmpc_handle* h, int32_t batch, const qmpc_convex_input* d_in,
                                     double* d_forces_world, qmpc_info* d_info, void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_in || !d_forces_world))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != QMPC_MODEL_CONVEX) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  return launch_solve(h, batch, reinterpret_cast<const qmpc_input*>(d_in), d_forces_world, d_info, nullptr, nullptr, s);
}

static void finish_pending(qmpc_handle* h);
qmpc_status qmpc_wait(qmpc_handle* h) {
  if (!h) return QMPC_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(h->device));
  if (h->timed) HIP_TRY(hipEventSynchronize(h->ev1));
  HIP_TRY(hipStreamSynchronize(h->stream));
  finish_pending(h);          // zero-copy host call into pageable buffers: the copy-out it still owes
  h->stage_in_busy = 0;
  return QMPC_OK;
}

qmpc_status qmpc_last_kernel_ms(qmpc_handle* h, float* ms) {
  if (!h || !ms) return QMPC_BAD_ARGUMENT;
  if (!h->timed) { *ms = 0.0f; return QMPC_OK; }
  HIP_TRY(hipEventSynchronize(h->ev1));
  HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return QMPC_OK;
}

// What kind of memory is p?  1: host memory the device can address (hipHostMalloc / hipHostRegister / qmpc_host_alloc; *dev =
// its device-side alias), 2: device (or managed) memory -- a caller that hands a host-buffer entry point such a pointer gets
// the explicit-copy path, which takes any kind --, 0: pageable host memory (or unknown to the runtime)
static int pointer_kind(const void* p, void** dev) {
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (a.type == hipMemoryTypeHost && a.devicePointer) { *dev = a.devicePointer; return 1; }
  if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeArray) return 2;
  return 0;
}
static qmpc_status ensure_stage(qmpc_handle* h, int nl) {
  if (h->h_stage_in) return QMPC_OK;
  const size_t rec = sizeof(double) * (32 + 4 * nl), out = sizeof(double) * 3 * nl + sizeof(qmpc_info);
  void *a = nullptr, *b = nullptr;
  if (hipHostMalloc(&a, rec * (size_t)h->max_batch, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc(&b, out * (size_t)h->max_batch, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    if (a) (void)hipHostFree(a);
    h->zero_copy = 0;            // no pinned memory to be had: the copies below take the runtime's own staging
    return QMPC_OK;
  }
  h->h_stage_in = static_cast<unsigned char*>(a);
  h->h_stage_out = static_cast<unsigned char*>(b);
  return QMPC_OK;
}
// copy-out owed to a pageable caller of the zero-copy path (after the stream has drained)
static void finish_pending(qmpc_handle* h) {
  if (h->pending.forces) std::memcpy(h->pending.forces, h->h_stage_out, h->pending.fbytes);
  if (h->pending.info) std::memcpy(h->pending.info, h->h_stage_out + h->pending.fbytes, h->pending.ibytes);
  h->pending.forces = nullptr;
  h->pending.info = nullptr;
}

// host-buffer solve shared by the models (nx = doubles per state in traj_x).
// Batches that take a wave-per-instance kernel run ZERO-COPY (see qmpc_handle): records are read from, forces and status
// written to, host memory the device can address -- the caller's own buffers when they are pinned (qmpc_host_alloc,
// hipHostMalloc, hipHostRegister), the handle's pinned staging otherwise (one memcpy in, one out).  Lane-kernel batches
// (which sort and re-read their records) and calls that want trajectories keep explicit copies on the handle's stream.
static qmpc_status solve_host(qmpc_handle* h, int32_t batch, const qmpc_input* in, double* forces_body,
                              qmpc_info* info, double* traj_u, double* traj_x, int model, int nx,
                              bool blocking = true) {
  if (!h || batch < 0 || (batch > 0 && (!in || !forces_body))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != model) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  HIP_TRY(hipSetDevice(h->device));
  // an earlier qmpc_solve_async was never waited for: complete it first -- it owes a pageable caller its copy-out, or its
  // kernel may still be reading records out of the staging this call is about to refill
  if (h->pending.forces || h->pending.info || h->stage_in_busy) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    finish_pending(h);
    h->stage_in_busy = 0;
  }
  const int N = h->params.horizon;
  const int nl = model_nl(model), nu = 3 * nl;
  const size_t rec = sizeof(double) * (32 + 4 * nl);
  const size_t fbytes = sizeof(double) * nu * (size_t)batch, ibytes = sizeof(qmpc_info) * (size_t)batch;
  if (traj_u && !h->d_traj_u) HIP_TRY(hipMalloc(&h->d_traj_u, sizeof(double) * nu * N * (size_t)h->max_batch));
  if (traj_x && !h->d_traj_x) HIP_TRY(hipMalloc(&h->d_traj_x, sizeof(double) * 13 * (N + 1) * (size_t)h->max_batch));
  const bool lane = plan(h->sel, batch, QMPC_CALL_PLAIN, true, h->opts.handoff_failed).variant == 4;
  if (h->zero_copy && !lane) {
    void *din = nullptr, *df = nullptr, *di = nullptr;
    const int k_in = pointer_kind(in, &din), k_f = pointer_kind(forces_body, &df), k_i = info ? pointer_kind(info, &di) : 1;
    const bool in_pinned = k_in == 1, out_pinned = k_f == 1 && k_i == 1;
    const bool any_device = k_in == 2 || k_f == 2 || k_i == 2;      // not host buffers at all: the copy path below takes them
    if (!any_device && (!in_pinned || !out_pinned)) {
      const qmpc_status es = ensure_stage(h, nl);
      if (es != QMPC_OK) return es;
    }
    if (h->zero_copy && !any_device) {
      if (!in_pinned) { std::memcpy(h->h_stage_in, in, rec * (size_t)batch); din = h->h_stage_in; }
      if (!out_pinned) { df = h->h_stage_out; di = h->h_stage_out + fbytes; }
      const qmpc_status st = launch_solve(h, batch, static_cast<const qmpc_input*>(din), static_cast<double*>(df),
                                          info ? static_cast<qmpc_info*>(di) : h->d_info, traj_u ? h->d_traj_u : nullptr,
                                          traj_x ? h->d_traj_x : nullptr, h->stream);
      if (st != QMPC_OK) return st;
      if (traj_u) HIP_TRY(hipMemcpyAsync(traj_u, h->d_traj_u, sizeof(double) * nu * N * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
      if (traj_x) HIP_TRY(hipMemcpyAsync(traj_x, h->d_traj_x, sizeof(double) * nx * (N + 1) * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
      if (!out_pinned) {
        h->pending.forces = forces_body; h->pending.fbytes = fbytes;
        h->pending.info = info; h->pending.ibytes = ibytes;
      }
      if (blocking) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        finish_pending(h);
      } else if (!in_pinned) {
        h->stage_in_busy = 1;
      }
      return QMPC_OK;
    }
  }
  HIP_TRY(hipMemcpyAsync(h->d_in, in, rec * (size_t)batch, hipMemcpyDefault, h->stream));
  const qmpc_status st = launch_solve(h, batch, h->d_in, h->d_forces, h->d_info, traj_u ? h->d_traj_u : nullptr,
                                      traj_x ? h->d_traj_x : nullptr, h->stream);
  if (st != QMPC_OK) return st;
  HIP_TRY(hipMemcpyAsync(forces_body, h->d_forces, fbytes, hipMemcpyDefault, h->stream));
  if (info) HIP_TRY(hipMemcpyAsync(info, h->d_info, ibytes, hipMemcpyDefault, h->stream));
  if (traj_u) HIP_TRY(hipMemcpyAsync(traj_u, h->d_traj_u, sizeof(double) * nu * N * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  if (traj_x) HIP_TRY(hipMemcpyAsync(traj_x, h->d_traj_x, sizeof(double) * nx * (N + 1) * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  if (blocking) HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

// ---- warm-started solve (converged mode, QuatMpc): every instance starts from u_init shifted by one knot ----------------
qmpc_status qmpc_solve_warm_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in, const double* d_u_init,
                                   double* d_forces_body, qmpc_info* d_info, double* d_traj_u, void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_in || !d_forces_body))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != QMPC_MODEL_QUAT || h->params.mode != QMPC_MODE_CONVERGED) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const qmpc_plan p = plan(h->sel, batch, QMPC_CALL_WARM, true, h->opts.handoff_failed);
  if (p.variant == 4) {      // large batches: the lane-per-instance kernel, same start rule
    const qmpc_status es = ensure_lane_buffers(h);
    if (es != QMPC_OK) return es;
    return launch_lane(h, p, batch, d_in, d_forces_body, d_info, s, d_u_init, d_traj_u, 0, nullptr, false);
  }
  HIP_TRY(qmpc_warm_launch(p.variant, 0, (int)batch, p.lds, s, &h->dev, sizeof h->dev, d_in, d_u_init, d_forces_body, d_info, d_traj_u,
                           p.gws ? h->d_gws : nullptr, 0));
  return QMPC_OK;
}

qmpc_status qmpc_solve_warm(qmpc_handle* h, int32_t batch, const qmpc_input* in, const double* u_init, double* forces_body,
                            qmpc_info* info, double* traj_u) {
  if (!h || batch < 0 || (batch > 0 && (!in || !forces_body))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != QMPC_MODEL_QUAT || h->params.mode != QMPC_MODE_CONVERGED) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  HIP_TRY(hipSetDevice(h->device));
  const int N = h->params.horizon;
  const size_t nu = sizeof(double) * 12 * N * (size_t)batch;
  // the device trajectory buffer doubles as the staging of u_init (read before it is overwritten: one wave per instance
  // loads its slice into LDS first)
  if (!h->d_traj_u) HIP_TRY(hipMalloc(&h->d_traj_u, sizeof(double) * 12 * N * (size_t)h->max_batch));
  HIP_TRY(hipMemcpyAsync(h->d_in, in, sizeof(qmpc_input) * (size_t)batch, hipMemcpyHostToDevice, h->stream));
  if (u_init) HIP_TRY(hipMemcpyAsync(h->d_traj_u, u_init, nu, hipMemcpyHostToDevice, h->stream));
  const qmpc_status st = qmpc_solve_warm_device(h, batch, h->d_in, u_init ? h->d_traj_u : nullptr, h->d_forces, h->d_info,
                                                h->d_traj_u, h->stream);
  if (st != QMPC_OK) return st;
  HIP_TRY(hipMemcpyAsync(forces_body, h->d_forces, sizeof(double) * 12 * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  if (info) HIP_TRY(hipMemcpyAsync(info, h->d_info, sizeof(qmpc_info) * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  if (traj_u) HIP_TRY(hipMemcpyAsync(traj_u, h->d_traj_u, nu, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

// non-blocking host-buffer call: copies and kernel are queued on the handle's stream; qmpc_wait completes them
qmpc_status qmpc_solve_async(qmpc_handle* h, int32_t batch, const qmpc_input* in, double* forces_body, qmpc_info* info) {
  return solve_host(h, batch, in, forces_body, info, nullptr, nullptr, QMPC_MODEL_QUAT, 13, false);
}

qmpc_status qmpc_solve_traj(qmpc_handle* h, int32_t batch, const qmpc_input* in, double* forces_body,
                            qmpc_info* info, double* traj_u, double* traj_x) {
  return solve_host(h, batch, in, forces_body, info, traj_u, traj_x, QMPC_MODEL_QUAT, 13);
}

qmpc_status qmpc_solve8_traj(qmpc_handle* h, int32_t batch, const qmpc_input8* in, double* forces_body,
                             qmpc_info* info, double* traj_u, double* traj_x) {
  return solve_host(h, batch, reinterpret_cast<const qmpc_input*>(in), forces_body, info, traj_u, traj_x,
                    QMPC_MODEL_QUAT8, 13);
}

qmpc_status qmpc_solve8(qmpc_handle* h, int32_t batch, const qmpc_input8* in, double* forces_body, qmpc_info* info) {
  return qmpc_solve8_traj(h, batch, in, forces_body, info, nullptr, nullptr);
}

qmpc_status qmpc_convex_solve_traj(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in, double* forces_world,
                                   qmpc_info* info, double* traj_u, double* traj_x) {
  return solve_host(h, batch, reinterpret_cast<const qmpc_input*>(in), forces_world, info, traj_u, traj_x,
                    QMPC_MODEL_CONVEX, 12);
}

qmpc_status qmpc_convex_solve(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in, double* forces_world,
                              qmpc_info* info) {
  return qmpc_convex_solve_traj(h, batch, in, forces_world, info, nullptr, nullptr);
}

qmpc_status qmpc_solve(qmpc_handle* h, int32_t batch, const qmpc_input* in, double* forces_body, qmpc_info* info) {
  return qmpc_solve_traj(h, batch, in, forces_body, info, nullptr, nullptr);
}

static qmpc_status linearize_host(qmpc_handle* h, int32_t batch, const qmpc_input* in, double* Abar, double* Bbar,
                                  double* X, int model, int nx) {
  if (!h || batch < 0 || (batch > 0 && (!in || !Abar || !Bbar || !X))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != model) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  HIP_TRY(hipSetDevice(h->device));
  const int N = h->params.horizon;
  const size_t nA = sizeof(double) * 144 * N * (size_t)h->max_batch;
  if (!h->d_A) HIP_TRY(hipMalloc(&h->d_A, nA));
  if (!h->d_B) HIP_TRY(hipMalloc(&h->d_B, nA));
  if (!h->d_traj_x) HIP_TRY(hipMalloc(&h->d_traj_x, sizeof(double) * 13 * (N + 1) * (size_t)h->max_batch));
  HIP_TRY(hipMemcpyAsync(h->d_in, in, sizeof(qmpc_input) * (size_t)batch, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(kLinearize[linearize_slot(model)], dim3((unsigned)batch), dim3(kWave), h->sel.lds[0][1], h->stream, h->dev, h->d_in,
                     h->d_A, h->d_B, h->d_traj_x, (int)batch);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(Abar, h->d_A, sizeof(double) * 144 * N * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(Bbar, h->d_B, sizeof(double) * 144 * N * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(X, h->d_traj_x, sizeof(double) * nx * (N + 1) * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

qmpc_status qmpc_linearize(qmpc_handle* h, int32_t batch, const qmpc_input* in, double* Abar, double* Bbar, double* X) {
  return linearize_host(h, batch, in, Abar, Bbar, X, QMPC_MODEL_QUAT, 13);
}

qmpc_status qmpc_convex_linearize(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in, double* A, double* B,
                                  double* X) {
  return linearize_host(h, batch, reinterpret_cast<const qmpc_input*>(in), A, B, X, QMPC_MODEL_CONVEX, 12);
}

// ---- pinned host buffers, eager allocation, handle queries ------------------------------------------------------------------
void* qmpc_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void qmpc_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

// the handle hands the stragglers of capped lane launches over (plain solves, cold- or warm-started loops)
static bool handoff_active(const qmpc_handle* h) {
  return lane_cap(h->sel, QMPC_CALL_PLAIN, h->opts.handoff_failed) || lane_cap(h->sel, QMPC_CALL_LOOP_TICK, h->opts.handoff_failed) ||
         lane_cap(h->sel, QMPC_CALL_WARM_LOOP_TICK, h->opts.handoff_failed);
}

static qmpc_status ensure_instance_buffers(qmpc_handle* h);
static qmpc_status ensure_lane_inst_buffers(qmpc_handle* h, bool handoff);
static qmpc_status ensure_plant_buffers(qmpc_handle* h);
// the buffers of a call with per-instance records where `p` plans it on the lane kernel (QMPC_INSTANCES_AUTO): the per-instance
// blocks, for a loop the plant blocks, the lane kernel's buffers and, where the plan hands stragglers over, the hand-off records
static qmpc_status prepare_lane_inst(qmpc_handle* h, const qmpc_plan& p, bool loop) {
  if (p.variant != 4) return QMPC_OK;
  qmpc_status es = ensure_instance_buffers(h);
  if (es == QMPC_OK && loop) es = ensure_plant_buffers(h);
  if (es == QMPC_OK) es = ensure_lane_inst_buffers(h, p.iter_cap != 0);
  return es;
}

// Everything a solve of `batch` instances will need, allocated NOW: the lane kernel's workspace and sort scratch, the
// hand-off records, the pinned staging of the host-buffer calls.  Afterwards no solve of up to `batch` instances allocates
// (safe inside the caller's own stream capture) and qmpc_query(QMPC_QUERY_HANDOFF_ACTIVE) says which family of roundings
// the handle's large-batch results belong to.
qmpc_status qmpc_prepare(qmpc_handle* h, int32_t batch) {
  if (!h || batch < 1) return QMPC_BAD_ARGUMENT;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  HIP_TRY(hipSetDevice(h->device));
  // the lane kernel's buffers where a plain solve or a cold-started loop's tick of this size takes it; the hand-off records
  // wherever the handle hands stragglers over at all
  if (plan(h->sel, batch, QMPC_CALL_PLAIN, true, h->opts.handoff_failed).variant == 4 ||
      plan(h->sel, batch, QMPC_CALL_LOOP_TICK, true, h->opts.handoff_failed).variant == 4) {
    const qmpc_status es = ensure_lane_buffers(h);
    if (es != QMPC_OK) return es;
    if (handoff_active(h)) (void)ensure_handoff_buffers(h);
  }
  // ... and where qmpc_solve_instances* of this size or the ticks of qmpc_loop_run_instances* / qmpc_loop_run_outcomes* with
  // controller records (cold-started; warm-started on a handle that opted in) take the lane kernel with per-lane parameters
  qmpc_status ps = prepare_lane_inst(h, plan_instances(h->sel, h->opts, batch, /*has_info=*/true), false);
  // (ConvexMpc: on a handle that opted in to the lane form, qmpc_set_convex_lane_records)
  if (ps == QMPC_OK) ps = prepare_lane_inst(h, plan_convex_instances(h->sel, h->opts, batch, /*has_info=*/true), false);
  for (int warm = 0; warm < 2 && ps == QMPC_OK; ++warm)
    ps = prepare_lane_inst(h, plan_loop_instances(h->sel, h->opts, batch, /*has_ctrl=*/true, warm != 0), true);
  if (ps != QMPC_OK) return ps;
  // the pinned staging of the host-buffer calls: ALWAYS (a handle prepared for a lane-kernel batch may still be handed a smaller
  // batch on host buffers, which runs zero-copy), and the buffers the closed loops and the trajectory / warm-started calls
  // otherwise allocate on first use -- nothing of that may happen inside a caller's stream capture
  if (h->zero_copy) {
    const qmpc_status es = ensure_stage(h, model_nl(h->params.model));
    if (es != QMPC_OK) return es;
  }
  const int nu = 3 * model_nl(h->params.model), N = h->params.horizon;
  if (!h->d_traj_u) HIP_TRY(hipMalloc(&h->d_traj_u, sizeof(double) * nu * N * (size_t)h->max_batch));
  if (!h->d_traj_x) HIP_TRY(hipMalloc(&h->d_traj_x, sizeof(double) * 13 * (N + 1) * (size_t)h->max_batch));
  if (!h->d_loop_row) HIP_TRY(hipMalloc(&h->d_loop_row, sizeof(int) * 4));
  return QMPC_OK;
}

// ---- per-instance robot and cost parameters (QuatMpc, converged mode; qmpc_wform.hip: qmpc_solve_w_inst_kernel) -------------
static_assert(sizeof(qmpc_instance_params) == 38 * sizeof(double), "qmpc_instance_params is 38 doubles");
int32_t qmpc_sizeof_instance_params(void) { return (int32_t)sizeof(qmpc_instance_params); }

void qmpc_instance_params_from(const qmpc_params* p, qmpc_instance_params* out) {
  if (!p || !out) return;
  out->mass = p->mass;
  std::memcpy(out->inertia, p->inertia, sizeof out->inertia);
  out->mu = p->mu;
  out->fz_max = p->fz_max;
  std::memcpy(out->q_weights, p->q_weights, sizeof out->q_weights);
  std::memcpy(out->r_weights, p->r_weights, sizeof out->r_weights);
  out->w = p->w;
}

static size_t instance_bytes(int max_batch) {
  return (sizeof(DevParams) + sizeof(qmpc_instance_params) + sizeof(int)) * (size_t)max_batch;
}
static qmpc_status ensure_instance_buffers(qmpc_handle* h) {
  if (!h->d_inst) HIP_TRY(hipMalloc(&h->d_inst, instance_bytes(h->max_batch)));
  return QMPC_OK;
}
static DevParams* inst_dev(qmpc_handle* h) { return reinterpret_cast<DevParams*>(h->d_inst); }
// ... and the per-robot plants of the closed loop (qmpc_loop_run_instances*), on its first use (a call with ticks = 0 allocates
// them and launches nothing)
static_assert(sizeof(qmpc_plant_params) == 16 * sizeof(double), "qmpc_plant_params is 16 doubles");
static_assert(sizeof(PlantDev) == 136, "PlantDev: 16 doubles and the verdict");
static size_t plant_bytes(int max_batch) { return (sizeof(PlantDev) + sizeof(qmpc_plant_params)) * (size_t)max_batch; }
static qmpc_status ensure_plant_buffers(qmpc_handle* h) {
  if (!h->d_plant) HIP_TRY(hipMalloc(&h->d_plant, plant_bytes(h->max_batch)));
  return QMPC_OK;
}
static PlantDev* plant_dev(qmpc_handle* h) { return reinterpret_cast<PlantDev*>(h->d_plant); }
static qmpc_plant_params* plant_rec(qmpc_handle* h) {
  return reinterpret_cast<qmpc_plant_params*>(h->d_plant + sizeof(PlantDev) * (size_t)h->max_batch);
}
static qmpc_instance_params* inst_rec(qmpc_handle* h) {
  return reinterpret_cast<qmpc_instance_params*>(h->d_inst + sizeof(DevParams) * (size_t)h->max_batch);
}
static int* inst_status(qmpc_handle* h) {
  return reinterpret_cast<int*>(h->d_inst + (sizeof(DevParams) + sizeof(qmpc_instance_params)) * (size_t)h->max_batch);
}

// The solves with per-instance parameters come in two models, QuatMpc's (qmpc_solve_instances*) and ConvexMpc's
// (qmpc_convex_solve_instances*; qmpc_wform_cinst.hip: qmpc_solve_cw_inst_kernel).  The records, the expansion kernel and the
// handle's per-instance buffers are the same: apply_instance_params writes the record's fields into the handle's DevParams
// whatever the model.  `convex` says which of the two a call is; the plan of a call:
static qmpc_plan plan_inst_call(const qmpc_handle* h, bool convex, int batch, bool has_info) {
  return convex ? plan_convex_instances(h->sel, h->opts, batch, has_info) : plan_instances(h->sel, h->opts, batch, has_info);
}
// the call-level checks both entry points share (after the null-pointer ones)
static qmpc_status instances_check(const qmpc_handle* h, bool convex, int32_t batch) {
  if (h->params.model != (convex ? QMPC_MODEL_CONVEX : QMPC_MODEL_QUAT) || h->params.mode != QMPC_MODE_CONVERGED) return QMPC_UNSUPPORTED;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  if (batch > 0 && plan_inst_call(h, convex, batch, true).family == QMPC_KERNEL_NONE) return QMPC_UNSUPPORTED;
  return QMPC_OK;
}

// the lane kernel's buffers for per-instance records (QMPC_INSTANCES_AUTO): the plain lane kernel's workspace and sort scratch,
// the parameter blocks of the resident wavefronts and, where the handle hands stragglers over, the hand-off records
static qmpc_status ensure_lane_inst_buffers(qmpc_handle* h, bool handoff) {
  const qmpc_status es = ensure_lane_buffers(h);
  if (es != QMPC_OK) return es;
  if (!h->d_lane_prm) HIP_TRY(hipMalloc(&h->d_lane_prm, qmpc_lane_inst_param_bytes(h->lane_slots)));
  if (handoff) (void)ensure_handoff_buffers(h);
  return QMPC_OK;
}
// some batch of the handle takes the lane kernel in qmpc_solve_instances* (ConvexMpc: qmpc_convex_solve_instances*) under its
// current settings
static bool instances_lane_possible(const qmpc_handle* h) {
  return plan_inst_call(h, h->params.model == QMPC_MODEL_CONVEX, h->max_batch, true).variant == 4;
}

// The solve of one call or tick with per-instance parameters, as `p` plans it (the blocks expanded and the buffers allocated
// already): d_in -> d_forces, d_info, and the trajectories where tu / tx are given.  Nothing here but kernels, the plain call's
// parameter upload and the hand-off counter's memset, so a tick can be captured.
//   INST_CALL        qmpc_solve_instances* / qmpc_convex_solve_instances*
//   INST_TICK_COLD   a tick of a cold-started loop with controller records
//   INST_TICK_FIRST  the cold first tick of a warm-started one (p: the plan with `first`), leaving its solution in tu
//   INST_TICK_WARM   ... its later ticks: the warm-started kernels start from tu (a robot whose previous solve failed starts cold:
//                    check_prev) and leave theirs there
// The wave form: the per-instance wrench-form kernel of the model.  The lane form, one path through kLaneInst[convex]: the sort --
// the plain call's by stance mask (QuatMpc: unit 1's, ConvexMpc: its unit's with the contacts at the convex record's offset), a
// tick's also by the previous records' iteration classes, robots that will not solve last --, the plain call's upload of the
// lane kernel's parameter block (the loops upload it once per call, outside the capture), the lane kernel with per-lane
// parameters of the model and start and, for QuatMpc with a cap, the per-instance list kernel on what it leaves (a warm tick's
// records carry the rows' initial residuals, so only the cold forms honour QMPC_HANDOFF_RESTART).  ConvexMpc's kernels have
// neither cap nor hand-off.
enum inst_form { INST_CALL, INST_TICK_COLD, INST_TICK_FIRST, INST_TICK_WARM };
static qmpc_status inst_solve(qmpc_handle* h, const qmpc_plan& p, bool convex, inst_form form, int32_t batch, const qmpc_input* d_in,
                              double* d_forces, qmpc_info* d_info, double* tu, double* tx, hipStream_t s) {
  const bool warm = form == INST_TICK_WARM;
  double* gws = p.gws ? h->d_gws : nullptr;
  if (p.variant == 4) {
    const auto& L = kLaneInst[convex].start[warm];
    const bool cap = !convex && p.iter_cap > 0;
    const int* perm = h->sel.lane_sort ? h->d_lane_scratch + 512 : nullptr;
    int *hcount = cap ? h->d_handoff : nullptr, *hsel = cap ? h->d_handoff + 64 : nullptr;
    double* hstate = cap ? h->d_hstate : nullptr;
    if (h->sel.lane_sort && form == INST_CALL && !convex) HIP_TRY(qmpc_lane_sort_launch((int)batch, s, d_in, h->d_lane_scratch));
    else if (h->sel.lane_sort)
      HIP_TRY(kLaneInst[convex].sort_launch((int)batch, s, d_in, (form != INST_CALL && p.order_prev) ? d_info : nullptr, inst_status(h),
                                            form != INST_CALL ? h->sel.lane_sort_idle : 0, h->d_lane_scratch));
    if (form == INST_CALL) HIP_TRY(L.upload_params(h->lane_pslot, s, &h->dev, sizeof h->dev));
    HIP_TRY(L.launch_only(h->lane_pslot, (int)batch, s, d_in, inst_dev(h), inst_status(h), d_forces, d_info, h->d_lane_ws, h->d_lane_prm,
                          h->lane_slots, perm, warm ? tu : nullptr, tu, tx, /*check_prev=*/1, p.iter_cap, hcount, hsel, hstate,
                          h->hstate_cap, h->sel.lane_pair));
    if (cap)
      HIP_TRY(qmpc_wform_inst_list_launch(p.handoff_variant, p.handoff_grid, p.lds, s, inst_dev(h), d_in, d_forces, d_info, tu, tx, hsel, hcount,
                                          gws, (warm || !h->sel.handoff_restart) ? h->d_hstate : nullptr, h->hstate_cap));
  } else if (convex && warm) {
    HIP_TRY(qmpc_wform_cinst_warm_launch(p.variant, (int)batch, p.lds, s, inst_dev(h), inst_status(h), d_in, tu, d_forces, d_info, tu, gws,
                                         /*check_prev=*/1));
  } else if (convex) {
    HIP_TRY(qmpc_wform_cinst_solve_launch(p.variant, (int)batch, p.lds, s, inst_dev(h), inst_status(h), d_in, d_forces, d_info, tu, tx, gws));
  } else if (warm) {
    HIP_TRY(qmpc_wform_inst_warm_launch(p.variant, (int)batch, p.lds, s, inst_dev(h), inst_status(h), d_in, tu, d_forces, d_info, tu, gws,
                                        /*check_prev=*/1));
  } else {
    HIP_TRY(qmpc_wform_inst_solve_launch(p.variant, (int)batch, p.lds, s, inst_dev(h), inst_status(h), d_in, d_forces, d_info, tu, tx, gws));
  }
  h->last_kernel = p.family;
  return QMPC_OK;
}

// expansion kernel + solve on stream s; d_rec: the records in device-addressable memory
static qmpc_status launch_instances(qmpc_handle* h, bool convex, int32_t batch, const qmpc_input* d_in, const qmpc_instance_params* d_rec,
                                    double* d_forces, qmpc_info* d_info, double* d_tu, double* d_tx, hipStream_t s) {
  qmpc_plan p = plan_inst_call(h, convex, batch, d_info != nullptr);
  const qmpc_status es = ensure_instance_buffers(h);
  if (es != QMPC_OK) return es;
  if (p.variant == 4) {
    const qmpc_status ls = ensure_lane_inst_buffers(h, false);
    if (ls != QMPC_OK) return ls;
    // (the hand-off records are allocated on first use; without them the pure lane kernel)
    if (p.iter_cap && !ensure_handoff_buffers(h)) p = plan_inst_call(h, convex, batch, true);
  }
  HIP_TRY(hipEventRecord(h->ev0, s));
  HIP_TRY(qmpc_wform_inst_expand_launch((int)batch, s, &h->dev, sizeof h->dev, d_rec, inst_dev(h), inst_status(h)));
  const qmpc_status st = inst_solve(h, p, convex, INST_CALL, batch, d_in, d_forces, d_info, d_tu, d_tx, s);
  if (st != QMPC_OK) return st;
  HIP_TRY(hipEventRecord(h->ev1, s));
  h->timed = true;
  return QMPC_OK;
}

// the device-buffer entry points after their null-pointer checks
static qmpc_status solve_instances_device(qmpc_handle* h, bool convex, int32_t batch, const qmpc_input* d_in,
                                          const qmpc_instance_params* d_iparams, double* d_forces, qmpc_info* d_info, void* stream) {
  const qmpc_status cs = instances_check(h, convex, batch);
  if (cs != QMPC_OK || batch == 0) return cs;
  HIP_TRY(hipSetDevice(h->device));
  return launch_instances(h, convex, batch, d_in, d_iparams, d_forces, d_info, nullptr, nullptr, stream ? (hipStream_t)stream : h->stream);
}

// ... and the host-buffer ones.  The trajectory buffers are sized as every call of the handle sizes them (rows of 13 hold
// ConvexMpc's rows of 12); the copy-out of traj_x is the model's: 13 (N + 1) doubles per instance, ConvexMpc 12 (N + 1).
static qmpc_status solve_instances_host(qmpc_handle* h, bool convex, int32_t batch, const qmpc_input* in, const qmpc_instance_params* iparams,
                                        double* forces, qmpc_info* info, double* traj_u, double* traj_x) {
  const qmpc_status cs = instances_check(h, convex, batch);
  if (cs != QMPC_OK || batch == 0) return cs;
  HIP_TRY(hipSetDevice(h->device));
  // an earlier qmpc_solve_async was never waited for: complete it first (it owes a pageable caller its copy-out)
  if (h->pending.forces || h->pending.info || h->stage_in_busy) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    finish_pending(h);
    h->stage_in_busy = 0;
  }
  const int N = h->params.horizon, nx = convex ? 12 : 13;
  const qmpc_status es = ensure_instance_buffers(h);
  if (es != QMPC_OK) return es;
  if (traj_u && !h->d_traj_u) HIP_TRY(hipMalloc(&h->d_traj_u, sizeof(double) * 12 * N * (size_t)h->max_batch));
  if (traj_x && !h->d_traj_x) HIP_TRY(hipMalloc(&h->d_traj_x, sizeof(double) * 13 * (N + 1) * (size_t)h->max_batch));
  HIP_TRY(hipMemcpyAsync(h->d_in, in, sizeof(qmpc_input) * (size_t)batch, hipMemcpyDefault, h->stream));
  HIP_TRY(hipMemcpyAsync(inst_rec(h), iparams, sizeof(qmpc_instance_params) * (size_t)batch, hipMemcpyDefault, h->stream));
  const qmpc_status st = launch_instances(h, convex, batch, h->d_in, inst_rec(h), h->d_forces, h->d_info, traj_u ? h->d_traj_u : nullptr,
                                          traj_x ? h->d_traj_x : nullptr, h->stream);
  if (st != QMPC_OK) return st;
  HIP_TRY(hipMemcpyAsync(forces, h->d_forces, sizeof(double) * 12 * (size_t)batch, hipMemcpyDefault, h->stream));
  if (info) HIP_TRY(hipMemcpyAsync(info, h->d_info, sizeof(qmpc_info) * (size_t)batch, hipMemcpyDefault, h->stream));
  if (traj_u) HIP_TRY(hipMemcpyAsync(traj_u, h->d_traj_u, sizeof(double) * 12 * N * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  if (traj_x) HIP_TRY(hipMemcpyAsync(traj_x, h->d_traj_x, sizeof(double) * nx * (N + 1) * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

qmpc_status qmpc_solve_instances_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in, const qmpc_instance_params* d_iparams,
                                        double* d_forces_body, qmpc_info* d_info, void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_in || !d_iparams || !d_forces_body))) return QMPC_BAD_ARGUMENT;
  return solve_instances_device(h, false, batch, d_in, d_iparams, d_forces_body, d_info, stream);
}

qmpc_status qmpc_solve_instances(qmpc_handle* h, int32_t batch, const qmpc_input* in, const qmpc_instance_params* iparams,
                                 double* forces_body, qmpc_info* info, double* traj_u, double* traj_x) {
  if (!h || batch < 0 || (batch > 0 && (!in || !iparams || !forces_body))) return QMPC_BAD_ARGUMENT;
  return solve_instances_host(h, false, batch, in, iparams, forces_body, info, traj_u, traj_x);
}

qmpc_status qmpc_convex_solve_instances_device(qmpc_handle* h, int32_t batch, const qmpc_convex_input* d_in,
                                               const qmpc_instance_params* d_iparams, double* d_forces_world, qmpc_info* d_info,
                                               void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_in || !d_iparams || !d_forces_world))) return QMPC_BAD_ARGUMENT;
  return solve_instances_device(h, true, batch, reinterpret_cast<const qmpc_input*>(d_in), d_iparams, d_forces_world, d_info, stream);
}

qmpc_status qmpc_convex_solve_instances(qmpc_handle* h, int32_t batch, const qmpc_convex_input* in, const qmpc_instance_params* iparams,
                                        double* forces_world, qmpc_info* info, double* traj_u, double* traj_x) {
  if (!h || batch < 0 || (batch > 0 && (!in || !iparams || !forces_world))) return QMPC_BAD_ARGUMENT;
  return solve_instances_host(h, true, batch, reinterpret_cast<const qmpc_input*>(in), iparams, forces_world, info, traj_u, traj_x);
}

// ---- a contact schedule over the horizon (qmpc_wform_sched.hip: qmpc_solve_w_sched_kernel) -------------
// The buffers, the expansion kernel and the verdicts of qmpc_solve_instances*; the schedule is one more kernel argument.
static qmpc_status schedule_check(const qmpc_handle* h, int32_t batch) {
  if (h->params.model != QMPC_MODEL_QUAT || h->params.mode != QMPC_MODE_CONVERGED) return QMPC_UNSUPPORTED;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  if (batch > 0 && plan_schedule(h->sel, batch).family == QMPC_KERNEL_NONE) return QMPC_UNSUPPORTED;
  return QMPC_OK;
}
// expansion (the records, or the handle's own values once per call) + solve on stream s; everything in device-addressable memory
static qmpc_status launch_schedule(qmpc_handle* h, int32_t batch, const qmpc_input* d_in, const qmpc_instance_params* d_rec,
                                   const uint8_t* d_sched, double* d_forces, qmpc_info* d_info, double* d_tu, double* d_tx, hipStream_t s) {
  const qmpc_plan p = plan_schedule(h->sel, batch);
  const qmpc_status es = ensure_instance_buffers(h);
  if (es != QMPC_OK) return es;
  HIP_TRY(hipEventRecord(h->ev0, s));
  if (d_rec) {
    HIP_TRY(qmpc_wform_inst_expand_launch((int)batch, s, &h->dev, sizeof h->dev, d_rec, inst_dev(h), inst_status(h)));
  } else {
    qmpc_instance_params own;
    qmpc_instance_params_from(&h->params, &own);
    HIP_TRY(qmpc_wform_sched_expand_uniform_launch((int)batch, s, &h->dev, sizeof h->dev, &own, inst_dev(h), inst_status(h)));
  }
  HIP_TRY(qmpc_wform_sched_launch(p.variant, (int)batch, p.lds, s, inst_dev(h), inst_status(h), d_in, d_sched, d_forces, d_info, d_tu, d_tx,
                                  p.gws ? h->d_gws : nullptr));
  h->last_kernel = p.family;
  HIP_TRY(hipEventRecord(h->ev1, s));
  h->timed = true;
  return QMPC_OK;
}

qmpc_status qmpc_solve_schedule_device(qmpc_handle* h, int32_t batch, const qmpc_input* d_in, const qmpc_instance_params* d_iparams,
                                       const uint8_t* d_schedule, double* d_forces_body, qmpc_info* d_info, double* d_traj_u,
                                       double* d_traj_x, void* stream) {
  if (!h || batch < 0 || (batch > 0 && (!d_in || !d_schedule || !d_forces_body))) return QMPC_BAD_ARGUMENT;
  const qmpc_status cs = schedule_check(h, batch);
  if (cs != QMPC_OK || batch == 0) return cs;
  HIP_TRY(hipSetDevice(h->device));
  return launch_schedule(h, batch, d_in, d_iparams, d_schedule, d_forces_body, d_info, d_traj_u, d_traj_x,
                         stream ? (hipStream_t)stream : h->stream);
}

qmpc_status qmpc_solve_schedule(qmpc_handle* h, int32_t batch, const qmpc_input* in, const qmpc_instance_params* iparams,
                                const uint8_t* schedule, double* forces_body, qmpc_info* info, double* traj_u, double* traj_x) {
  if (!h || batch < 0 || (batch > 0 && (!in || !schedule || !forces_body))) return QMPC_BAD_ARGUMENT;
  const qmpc_status cs = schedule_check(h, batch);
  if (cs != QMPC_OK || batch == 0) return cs;
  HIP_TRY(hipSetDevice(h->device));
  // an earlier qmpc_solve_async was never waited for: complete it first (it owes a pageable caller its copy-out)
  if (h->pending.forces || h->pending.info || h->stage_in_busy) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    finish_pending(h);
    h->stage_in_busy = 0;
  }
  const int N = h->params.horizon;
  const qmpc_status es = ensure_instance_buffers(h);
  if (es != QMPC_OK) return es;
  if (!h->d_sched) HIP_TRY(hipMalloc(&h->d_sched, (size_t)N * (size_t)h->max_batch));
  if (traj_u && !h->d_traj_u) HIP_TRY(hipMalloc(&h->d_traj_u, sizeof(double) * 12 * N * (size_t)h->max_batch));
  if (traj_x && !h->d_traj_x) HIP_TRY(hipMalloc(&h->d_traj_x, sizeof(double) * 13 * (N + 1) * (size_t)h->max_batch));
  HIP_TRY(hipMemcpyAsync(h->d_in, in, sizeof(qmpc_input) * (size_t)batch, hipMemcpyDefault, h->stream));
  if (iparams) HIP_TRY(hipMemcpyAsync(inst_rec(h), iparams, sizeof(qmpc_instance_params) * (size_t)batch, hipMemcpyDefault, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_sched, schedule, (size_t)N * (size_t)batch, hipMemcpyDefault, h->stream));
  const qmpc_status st = launch_schedule(h, batch, h->d_in, iparams ? inst_rec(h) : nullptr, h->d_sched, h->d_forces, h->d_info,
                                         traj_u ? h->d_traj_u : nullptr, traj_x ? h->d_traj_x : nullptr, h->stream);
  if (st != QMPC_OK) return st;
  HIP_TRY(hipMemcpyAsync(forces_body, h->d_forces, sizeof(double) * 12 * (size_t)batch, hipMemcpyDefault, h->stream));
  if (info) HIP_TRY(hipMemcpyAsync(info, h->d_info, sizeof(qmpc_info) * (size_t)batch, hipMemcpyDefault, h->stream));
  if (traj_u) HIP_TRY(hipMemcpyAsync(traj_u, h->d_traj_u, sizeof(double) * 12 * N * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  if (traj_x) HIP_TRY(hipMemcpyAsync(traj_x, h->d_traj_x, sizeof(double) * 13 * (N + 1) * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

qmpc_status qmpc_prepare_instances(qmpc_handle* h) {
  if (!h) return QMPC_BAD_ARGUMENT;
  const bool convex = h->params.model == QMPC_MODEL_CONVEX;      // (ConvexMpc: the lane form on a handle that opted in only)
  const qmpc_status cs = instances_check(h, convex, 0);
  if (cs != QMPC_OK) return cs;
  HIP_TRY(hipSetDevice(h->device));
  const qmpc_status es = ensure_instance_buffers(h);
  // (a ConvexMpc handle that opted in to warm-started loops with controller records: the buffer the solution travels through in
  // the per-tick forms, 96 N bytes per robot)
  if (es == QMPC_OK && convex && h->opts.convex_records && h->opts.convex_warm && !h->d_traj_u)
    HIP_TRY(hipMalloc(&h->d_traj_u, sizeof(double) * 12 * (size_t)h->params.horizon * (size_t)h->max_batch));
  if (es != QMPC_OK || !instances_lane_possible(h)) return es;
  return ensure_lane_inst_buffers(h, lane_cap(h->sel, QMPC_CALL_PLAIN, h->opts.handoff_failed) != 0);
}

qmpc_status qmpc_set_instances_policy(qmpc_handle* h, int32_t policy) {
  if (!h || (policy != QMPC_INSTANCES_WAVE && policy != QMPC_INSTANCES_AUTO)) return QMPC_BAD_ARGUMENT;
  h->opts.inst_policy = policy;
  return QMPC_OK;
}

qmpc_status qmpc_set_loop_warm_records(qmpc_handle* h, int32_t on) {
  if (!h || (on != 0 && on != 1)) return QMPC_BAD_ARGUMENT;
  h->opts.loop_warm_records = on != 0;
  return QMPC_OK;
}

qmpc_status qmpc_set_convex_records(qmpc_handle* h, int32_t on) {
  if (!h || (on != 0 && on != 1)) return QMPC_BAD_ARGUMENT;
  h->opts.convex_records = on != 0;
  return QMPC_OK;
}

qmpc_status qmpc_set_convex_lane_records(qmpc_handle* h, int32_t on) {
  if (!h || (on != 0 && on != 1)) return QMPC_BAD_ARGUMENT;
  h->opts.convex_lane = on != 0;
  return QMPC_OK;
}

qmpc_status qmpc_set_convex_warm_records(qmpc_handle* h, int32_t on) {
  if (!h || (on != 0 && on != 1)) return QMPC_BAD_ARGUMENT;
  h->opts.convex_warm = on != 0;
  return QMPC_OK;
}

qmpc_status qmpc_query(qmpc_handle* h, int32_t what, int64_t arg, int64_t* value) {
  if (!h || !value) return QMPC_BAD_ARGUMENT;
  switch (what) {
    case QMPC_QUERY_HANDOFF_ACTIVE:      // 1: capped lane launches hand their stragglers over; 0: pure lane kernel (off, or allocation failed)
      *value = handoff_active(h) ? 1 : 0;
      return QMPC_OK;
    case QMPC_QUERY_HANDOFF_ALLOC_FAILED: *value = h->opts.handoff_failed; return QMPC_OK;
    case QMPC_QUERY_KERNEL_FOR_BATCH:
      if (arg < 1 || arg > h->max_batch) return QMPC_BAD_ARGUMENT;
      *value = plan(h->sel, (int)arg, QMPC_CALL_PLAIN, true, h->opts.handoff_failed).family;
      return QMPC_OK;
    case QMPC_QUERY_LAST_KERNEL: *value = h->last_kernel; return QMPC_OK;
    case QMPC_QUERY_LANE_CAP:
      *value = lane_cap(h->sel, arg == 3 ? QMPC_CALL_WARM_LOOP_TICK : (arg == 2 ? QMPC_CALL_LOOP_TICK : QMPC_CALL_PLAIN), h->opts.handoff_failed);
      return QMPC_OK;
    case QMPC_QUERY_DEVICE_BYTES: {      // device memory the handle holds right now
      const int N = h->params.horizon, nl = model_nl(h->params.model), nu = 3 * nl;
      size_t b = (sizeof(double) * (32 + 4 * nl) + sizeof(double) * nu + sizeof(qmpc_info)) * (size_t)h->max_batch;
      b += sizeof(double) * (size_t)N * (13 * nu + 21 * nl + 30 * nl) * (size_t)h->max_batch;
      if (h->d_lane_ws) b += qmpc_lane_ws_bytes(N, nl, h->lane_slots, h->params.mode == QMPC_MODE_REFERENCE) + qmpc_lane_scratch_bytes(h->max_batch);
      if (h->d_handoff) b += qmpc_lane_handoff_list_bytes(h->max_batch) + sizeof(double) * qmpc_lane_handoff_record_doubles(N) * (size_t)h->hstate_cap;
      if (h->d_traj_u) b += sizeof(double) * nu * N * (size_t)h->max_batch;
      if (h->d_traj_x) b += sizeof(double) * 13 * (N + 1) * (size_t)h->max_batch;
      if (h->d_A) b += 2 * sizeof(double) * 144 * N * (size_t)h->max_batch;
      if (h->d_inst) b += instance_bytes(h->max_batch);
      if (h->d_lane_prm) b += qmpc_lane_inst_param_bytes(h->lane_slots);
      if (h->d_plant) b += plant_bytes(h->max_batch);
      if (h->d_outcome) b += sizeof(qmpc_loop_outcome) * (size_t)h->max_batch;
      if (h->d_push) b += sizeof(qmpc_push_params) * (size_t)h->push_cap * (size_t)h->max_batch;
      for (const rec_stage& s : kRecStage)
        if (h->*s.buf) b += s.elem * (size_t)h->max_batch;
      if (h->d_sched) b += (size_t)N * (size_t)h->max_batch;
      b += sizeof(double) * (h->leg_cap + h->loop_cap);
      *value = (int64_t)b;
      return QMPC_OK;
    }
    case QMPC_QUERY_ZERO_COPY: *value = h->zero_copy; return QMPC_OK;
    case QMPC_QUERY_KERNEL_FOR_INSTANCES:
      if (arg < 1 || arg > h->max_batch) return QMPC_BAD_ARGUMENT;
      *value = plan_instances(h->sel, h->opts, (int)arg, true).family;
      return QMPC_OK;
    case QMPC_QUERY_INSTANCES_POLICY: *value = h->opts.inst_policy; return QMPC_OK;
    case QMPC_QUERY_LOOP_INSTANCES_PLAN: {
      const int64_t b = arg & 0xffffffffLL;
      if (b < 1 || b > h->max_batch) return QMPC_BAD_ARGUMENT;
      const qmpc_plan p = plan_loop_instances(h->sel, h->opts, (int)b, (arg >> 32) & 1, (arg >> 33) & 1);
      *value = p.family == QMPC_KERNEL_NONE ? 0 : 16 * (p.fused ? 1 : 2) + p.family;
      return QMPC_OK;
    }
    case QMPC_QUERY_LOOP_WARM_RECORDS: *value = h->opts.loop_warm_records; return QMPC_OK;
    case QMPC_QUERY_CONVEX_RECORDS: *value = h->opts.convex_records; return QMPC_OK;
    case QMPC_QUERY_KERNEL_FOR_CONVEX_INSTANCES:
      if (arg < 1 || arg > h->max_batch) return QMPC_BAD_ARGUMENT;
      *value = plan_convex_instances(h->sel, h->opts, (int)arg, true).family;
      return QMPC_OK;
    case QMPC_QUERY_CONVEX_LANE_RECORDS: *value = h->opts.convex_lane; return QMPC_OK;
    case QMPC_QUERY_CONVEX_WARM_RECORDS: *value = h->opts.convex_warm; return QMPC_OK;
    case QMPC_QUERY_KERNEL_FOR_SCHEDULE:
      if (arg < 1 || arg > h->max_batch) return QMPC_BAD_ARGUMENT;
      *value = plan_schedule(h->sel, (int)arg).family;
      return QMPC_OK;
    default: return QMPC_BAD_ARGUMENT;
  }
}

// ---- multi-GPU: the one collective of the path --------------------------------
// RCCL is resolved at run time (dlopen), so the library carries no link-time dependency on it and a
// single-GPU user never loads it.  ncclAllGather(sendbuff, recvbuff, sendcount, datatype, comm, stream);
// ncclFloat64 = 8 in nccl.h.
typedef int (*nccl_all_gather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static nccl_all_gather_fn resolve_all_gather() {
  static nccl_all_gather_fn fn = nullptr;
  static std::once_flag once;      // two handles may gather first from two threads
  std::call_once(once, [] {
    void* sym = dlsym(RTLD_DEFAULT, "ncclAllGather");          // already in the process (e.g. under torch)?
    if (!sym) {
      const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
      for (const char* n : names) {
        void* lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (lib && (sym = dlsym(lib, "ncclAllGather"))) break;
      }
    }
    fn = reinterpret_cast<nccl_all_gather_fn>(sym);
  });
  return fn;
}

qmpc_status qmpc_gather(qmpc_handle* h, void* nccl_comm, const double* d_local, int64_t count, double* d_all,
                        void* stream) {
  if (!h || !nccl_comm || count < 0 || (count > 0 && (!d_local || !d_all))) return QMPC_BAD_ARGUMENT;
  if (count == 0) return QMPC_OK;
  nccl_all_gather_fn fn = resolve_all_gather();
  if (!fn) {
    std::fprintf(stderr, "qmpc_gather: RCCL (ncclAllGather) not found\n");
    return QMPC_UNSUPPORTED;
  }
  HIP_TRY(hipSetDevice(h->device));
  const int rc = fn(d_local, d_all, (size_t)count, /*ncclFloat64*/ 8, nccl_comm, stream ? (hipStream_t)stream : h->stream);
  if (rc != 0) {
    std::fprintf(stderr, "qmpc_gather: ncclAllGather failed (%d)\n", rc);
    return QMPC_HIP_ERROR;
  }
  return QMPC_OK;
}

// ---- leg kinematics / torque map (BaseInterface.cpp:10-34,209-212,343-408) ----------------
void qmpc_default_go1_geometry(qmpc_leg_geometry* g) {
  std::memset(g, 0, sizeof *g);
  const double sx[4] = {1, 1, -1, -1}, sy[4] = {1, -1, 1, -1};
  for (int l = 0; l < 4; ++l) {
    g->rho_fix[l][0] = sx[l] * 0.1881;    // leg_offset_x
    g->rho_fix[l][1] = sy[l] * 0.04675;   // leg_offset_y
    g->rho_fix[l][2] = sy[l] * 0.0812;    // motor_offset
    g->rho_fix[l][3] = 0.213;             // UPPER_LEG_LENGTH
    g->rho_fix[l][4] = 0.213;             // LOWER_LEG_LENGTH
  }
}

static_assert(sizeof(LegGeom) == sizeof(qmpc_leg_geometry), "kernel argument mirrors the ABI struct");

static qmpc_status launch_leg(const qmpc_leg_geometry* g, int32_t batch, const double* d_q,
                              const double* d_f, const double* d_c, int walking, double* d_p, double* d_J,
                              double* d_tau, hipStream_t s) {
  LegGeom G;
  std::memcpy(&G, g, sizeof G);
  const bool aligned = ((reinterpret_cast<uintptr_t>(d_q) | reinterpret_cast<uintptr_t>(d_f) |
                         reinterpret_cast<uintptr_t>(d_tau)) & 15u) == 0;
  if (d_tau && !d_p && !d_J && aligned) {      // the torque map proper: LDS-staged streaming pass, 64 instances per block
    hipLaunchKernelGGL(qmpc_tau_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(256), 0, s, G, d_q, d_f, d_c, walking,
                       d_tau, (int)batch);
    HIP_TRY(hipGetLastError());
    return QMPC_OK;
  }
  const unsigned threads = 256, blocks = (unsigned)(((size_t)batch * 4 + threads - 1) / threads);
  hipLaunchKernelGGL(qmpc_leg_kernel, dim3(blocks), dim3(threads), 0, s, G, d_q, d_f, d_c, walking, d_p, d_J, d_tau,
                     (int)batch);
  HIP_TRY(hipGetLastError());
  return QMPC_OK;
}

qmpc_status qmpc_torque_map_device(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch, const double* d_joint_pos,
                                   const double* d_forces_body, const double* d_contacts, int32_t walking,
                                   double* d_tau, void* stream) {
  if (!h || !g || batch < 0 || (batch > 0 && (!d_joint_pos || !d_forces_body || !d_tau))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  return launch_leg(g, batch, d_joint_pos, d_forces_body, d_contacts, walking, nullptr, nullptr, d_tau,
                    stream ? (hipStream_t)stream : h->stream);
}

// host-buffer variants (not the hot path): staged through a buffer the handle keeps
static qmpc_status leg_host(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch, const double* q, const double* f,
                            const double* c, int walking, double* p, double* J, double* tau) {
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)batch;
  // layout: q[12B] f[12B] c[4B] p[12B] J[36B] tau[12B]; the staging buffer belongs to the handle and only grows
  if (h->leg_cap < B * 88) {
    if (h->d_leg) (void)hipFree(h->d_leg);
    h->d_leg = nullptr;
    h->leg_cap = 0;
    HIP_TRY(hipMalloc(&h->d_leg, sizeof(double) * B * 88));
    h->leg_cap = B * 88;
  }
  double* d = h->d_leg;
  double *dq = d, *df = d + 12 * B, *dc = d + 24 * B, *dp = d + 28 * B, *dJ = d + 40 * B, *dt = d + 76 * B;
  qmpc_status st = QMPC_OK;
  do {
    if (hipMemcpyAsync(dq, q, sizeof(double) * 12 * B, hipMemcpyHostToDevice, h->stream) != hipSuccess) { st = QMPC_HIP_ERROR; break; }
    if (f && hipMemcpyAsync(df, f, sizeof(double) * 12 * B, hipMemcpyHostToDevice, h->stream) != hipSuccess) { st = QMPC_HIP_ERROR; break; }
    if (c && hipMemcpyAsync(dc, c, sizeof(double) * 4 * B, hipMemcpyHostToDevice, h->stream) != hipSuccess) { st = QMPC_HIP_ERROR; break; }
    st = launch_leg(g, batch, dq, f ? df : nullptr, c ? dc : nullptr, walking, p ? dp : nullptr, J ? dJ : nullptr,
                    tau ? dt : nullptr, h->stream);
    if (st != QMPC_OK) break;
    if (p && hipMemcpyAsync(p, dp, sizeof(double) * 12 * B, hipMemcpyDeviceToHost, h->stream) != hipSuccess) { st = QMPC_HIP_ERROR; break; }
    if (J && hipMemcpyAsync(J, dJ, sizeof(double) * 36 * B, hipMemcpyDeviceToHost, h->stream) != hipSuccess) { st = QMPC_HIP_ERROR; break; }
    if (tau && hipMemcpyAsync(tau, dt, sizeof(double) * 12 * B, hipMemcpyDeviceToHost, h->stream) != hipSuccess) { st = QMPC_HIP_ERROR; break; }
    if (hipStreamSynchronize(h->stream) != hipSuccess) st = QMPC_HIP_ERROR;
  } while (0);
  return st;
}

qmpc_status qmpc_leg_kinematics(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch, const double* joint_pos,
                                double* foot_pos_body, double* jac) {
  if (!h || !g || batch < 0 || (batch > 0 && (!joint_pos || (!foot_pos_body && !jac)))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  return leg_host(h, g, batch, joint_pos, nullptr, nullptr, 0, foot_pos_body, jac, nullptr);
}

qmpc_status qmpc_torque_map(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch, const double* joint_pos,
                            const double* forces_body, const double* contacts, int32_t walking, double* tau) {
  if (!h || !g || batch < 0 || (batch > 0 && (!joint_pos || !forces_body || !tau))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  return leg_host(h, g, batch, joint_pos, forces_body, contacts, walking, nullptr, nullptr, tau);
}

// ---- joint-level commands (BaseInterface.cpp:343-408; kernels in qmpc_joint.hip) ------------------
static qmpc_status grow_leg_staging(qmpc_handle* h, size_t doubles) {
  if (h->leg_cap >= doubles) return QMPC_OK;
  if (h->d_leg) (void)hipFree(h->d_leg);
  h->d_leg = nullptr;
  h->leg_cap = 0;
  HIP_TRY(hipMalloc(&h->d_leg, sizeof(double) * doubles));
  h->leg_cap = doubles;
  return QMPC_OK;
}

qmpc_status qmpc_joint_commands_device(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                       const qmpc_joint_feedback* d_fb, qmpc_joint_command* d_cmd, void* stream) {
  if (!h || !g || batch < 0 || (batch > 0 && (!d_fb || !d_cmd))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  LegGeom G;
  std::memcpy(&G, g, sizeof G);
  hipLaunchKernelGGL(qmpc_joint_cmd_kernel, dim3((unsigned)((batch + kJointTile - 1) / kJointTile)), dim3(256), 0,
                     stream ? (hipStream_t)stream : h->stream, G, d_fb, d_cmd, (int)batch);
  HIP_TRY(hipGetLastError());
  return QMPC_OK;
}

qmpc_status qmpc_joint_commands(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch, const qmpc_joint_feedback* fb,
                                qmpc_joint_command* cmd) {
  if (!h || !g || batch < 0 || (batch > 0 && (!fb || !cmd))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)batch;
  const qmpc_status gs = grow_leg_staging(h, B * (kJointFb + kJointCmd));
  if (gs != QMPC_OK) return gs;
  qmpc_joint_feedback* dfb = reinterpret_cast<qmpc_joint_feedback*>(h->d_leg);
  qmpc_joint_command* dcmd = reinterpret_cast<qmpc_joint_command*>(h->d_leg + B * kJointFb);
  HIP_TRY(hipMemcpyAsync(dfb, fb, sizeof(qmpc_joint_feedback) * B, hipMemcpyHostToDevice, h->stream));
  const qmpc_status st = qmpc_joint_commands_device(h, g, batch, dfb, dcmd, h->stream);
  if (st != QMPC_OK) return st;
  HIP_TRY(hipMemcpyAsync(cmd, dcmd, sizeof(qmpc_joint_command) * B, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

qmpc_status qmpc_leg_inverse_kinematics(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                        const double* foot_pos_body, const double* cur_joint_pos, double* joint_pos) {
  if (!h || !g || batch < 0 || (batch > 0 && (!foot_pos_body || !cur_joint_pos || !joint_pos))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)batch;
  const qmpc_status gs = grow_leg_staging(h, B * 36);
  if (gs != QMPC_OK) return gs;
  double *dp = h->d_leg, *dc = h->d_leg + 12 * B, *dq = h->d_leg + 24 * B;
  HIP_TRY(hipMemcpyAsync(dp, foot_pos_body, sizeof(double) * 12 * B, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(dc, cur_joint_pos, sizeof(double) * 12 * B, hipMemcpyHostToDevice, h->stream));
  LegGeom G;
  std::memcpy(&G, g, sizeof G);
  hipLaunchKernelGGL(qmpc_leg_inverse_kernel, dim3((unsigned)((B * 4 + 255) / 256)), dim3(256), 0, h->stream, G,
                     (const double*)dp, (const double*)dc, dq, (int)batch);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(joint_pos, dq, sizeof(double) * 12 * B, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

qmpc_status qmpc_loop_joint_commands_device(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch,
                                            const qmpc_loop_state* d_states, double* d_joint_pos,
                                            qmpc_joint_feedback* d_fb, qmpc_joint_command* d_cmd, void* stream) {
  if (!h || !g || batch < 0 || (batch > 0 && (!d_states || !d_joint_pos || !d_cmd))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  LegGeom G;
  std::memcpy(&G, g, sizeof G);
  hipLaunchKernelGGL(qmpc_loop_joint_kernel, dim3((unsigned)(((size_t)batch * 4 + 255) / 256)), dim3(256), 0,
                     stream ? (hipStream_t)stream : h->stream, G, d_states, d_joint_pos, d_fb, d_cmd,
                     (qmpc_joint_command*)nullptr, (const int*)nullptr, (int)batch);
  HIP_TRY(hipGetLastError());
  return QMPC_OK;
}

// host-buffer form of the above (not the hot path): staged through temporaries
qmpc_status qmpc_loop_joint_commands(qmpc_handle* h, const qmpc_leg_geometry* g, int32_t batch, const qmpc_loop_state* states,
                                     double* joint_pos, qmpc_joint_feedback* fb, qmpc_joint_command* cmd) {
  if (!h || !g || batch < 0 || (batch > 0 && (!states || !joint_pos || !cmd))) return QMPC_BAD_ARGUMENT;
  if (batch == 0) return QMPC_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)batch;
  qmpc_loop_state* d_st = nullptr;
  qmpc_status rs = QMPC_OK;
  do {
    if (hipMalloc(&d_st, sizeof(qmpc_loop_state) * B) != hipSuccess) { rs = QMPC_HIP_ERROR; break; }
    rs = grow_leg_staging(h, B * (12 + kJointFb + kJointCmd));
    if (rs != QMPC_OK) break;
    double* d_jp = h->d_leg;
    qmpc_joint_feedback* d_fb = reinterpret_cast<qmpc_joint_feedback*>(h->d_leg + 12 * B);
    qmpc_joint_command* d_cmd = reinterpret_cast<qmpc_joint_command*>(h->d_leg + (12 + kJointFb) * B);
    if (hipMemcpyAsync(d_st, states, sizeof(qmpc_loop_state) * B, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(d_jp, joint_pos, sizeof(double) * 12 * B, hipMemcpyHostToDevice, h->stream) != hipSuccess) { rs = QMPC_HIP_ERROR; break; }
    rs = qmpc_loop_joint_commands_device(h, g, batch, d_st, d_jp, d_fb, d_cmd, h->stream);
    if (rs != QMPC_OK) break;
    if (hipMemcpyAsync(joint_pos, d_jp, sizeof(double) * 12 * B, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(cmd, d_cmd, sizeof(qmpc_joint_command) * B, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        (fb && hipMemcpyAsync(fb, d_fb, sizeof(qmpc_joint_feedback) * B, hipMemcpyDeviceToHost, h->stream) != hipSuccess)) { rs = QMPC_HIP_ERROR; break; }
    if (hipStreamSynchronize(h->stream) != hipSuccess) rs = QMPC_HIP_ERROR;
  } while (0);
  if (d_st) (void)hipFree(d_st);
  return rs;
}

void qmpc_loop_joint_init(double* joint_pos, int32_t batch) {
  const double stand[3] = {0.0, 0.67, -1.3};
  for (size_t t = 0; t < (size_t)(batch > 0 ? batch : 0) * 4; ++t)
    for (int j = 0; j < 3; ++j) joint_pos[3 * t + j] = stand[j];
}

// ---- device-resident closed loop (kernels in qmpc_loop.hip) ----------------
int32_t qmpc_sizeof_loop_state(void) { return (int32_t)sizeof(qmpc_loop_state); }
static_assert(sizeof(qmpc_loop_state) == 8 * 820, "qmpc_loop_state is 820 doubles");

void qmpc_default_loop_params(qmpc_loop_params* p) {
  std::memset(p, 0, sizeof *p);
  p->gait_freq = 2.2;                                               // LeggedState.h / yaml gait_freq
  const double f[4][3] = {{0.20, 0.14, -0.3}, {0.20, -0.14, -0.3}, {-0.20, 0.14, -0.3}, {-0.20, -0.14, -0.3}};
  for (int l = 0; l < 4; ++l)
    for (int a = 0; a < 3; ++a) p->default_foot_pos_rel[3 * l + a] = f[l][a];   // yaml default_foot_pos_*
  p->dt = 5.0 / 1000.0;
  p->contact_height = 1e-3;
}

void qmpc_loop_state_init(qmpc_loop_state* s, const qmpc_loop_params* lp, const double joy[6], double movement_mode,
                          double height, double yaw) {
  std::memset(s, 0, sizeof *s);
  s->pos_world[2] = height;
  s->quat[0] = std::cos(0.5 * yaw);
  s->quat[3] = std::sin(0.5 * yaw);
  double R[9], Rz[9];
  qmpc_loop::quat_to_rot(s->quat, R);
  qmpc_loop::rot_to_rot_z(R, Rz);
  for (int l = 0; l < 4; ++l)
    for (int r = 0; r < 3; ++r)
      s->foot_pos_world[3 * l + r] = Rz[3 * r] * lp->default_foot_pos_rel[3 * l] + Rz[3 * r + 1] * lp->default_foot_pos_rel[3 * l + 1] +
                                     Rz[3 * r + 2] * lp->default_foot_pos_rel[3 * l + 2] + s->pos_world[r];
  for (int a = 0; a < 6; ++a) s->joy[a] = joy[a];
  s->movement_mode = movement_mode;
  for (int a = 0; a < 3; ++a) s->pos_d_world[a] = s->pos_world[a];
  s->pos_d_init = 1.0;
  for (int a = 0; a < 4; ++a) s->quat_d[a] = s->quat[a];
  for (int l = 0; l < 4; ++l) {          // LeggedContactFSM::reset_params (:4-9) + set_default_gait_pattern
    qmpc_loop_leg& L = s->leg[l];
    L.state = 1.0;
    L.pattern_index = 0.0;
    L.prev_pattern_index = 1.0;
    L.start_time = 0.0;
    L.end_time = 0.5;
    s->contacts[l] = 1.0;
  }
}

// The solve of one tick of the closed loop in the per-tick form (h->d_in -> h->d_forces, h->d_info); first: the cold first
// tick of a warm-started call
static qmpc_status loop_tick_solve(qmpc_handle* h, int32_t batch, hipStream_t s, bool warm, bool first, bool convex) {
  if (warm) {
    const qmpc_plan p = plan(h->sel, batch, first ? QMPC_CALL_WARM_LOOP_FIRST : QMPC_CALL_WARM_LOOP_TICK, true, h->opts.handoff_failed);
    // the lane kernel hands the stragglers of the warm-started ticks over (not of the cold first one): the records carry the
    // rows' initial residuals
    if (p.variant == 4) {
      const qmpc_status st = launch_lane(h, p, batch, h->d_in, h->d_forces, h->d_info, s, first ? nullptr : h->d_traj_u, h->d_traj_u,
                                         /*check_prev=*/1, nullptr, false);
      if (st != QMPC_OK) return st;
    } else {
      HIP_TRY(qmpc_warm_launch(p.variant, convex ? 1 : 0, (int)batch, p.lds, s, &h->dev, sizeof h->dev, h->d_in, first ? nullptr : h->d_traj_u,
                               h->d_forces, h->d_info, h->d_traj_u, p.gws ? h->d_gws : nullptr, /*check_prev=*/1));
    }
    return QMPC_OK;
  }
  return launch_solve(h, batch, h->d_in, h->d_forces, h->d_info, nullptr, nullptr, s, QMPC_CALL_LOOP_TICK);
}

// the caller is capturing stream s into a graph of its own
static bool stream_is_capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cs == hipStreamCaptureStatusActive;
}

// The per-tick form of the closed loop: `one_tick(first)` enqueues one tick (three kernels, four with the joint level); it is
// captured once into a graph and replayed (the sequence is launch-bound for small batches); plain launches when capture is not
// available on this stream.  tick_plan: the plan of the solve of the tick the loop repeats.
extern "C++" {      // (a template, inside the extern "C" block of the entry points)
template <class Tick>
static qmpc_status replay_ticks(qmpc_handle* h, const qmpc_plan& tick_plan, hipStream_t s, int32_t ticks, bool warm, Tick&& one_tick) {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool captured = false;
  int t_start = 0;
  // Large batches solve with the lane-per-instance kernel in every tick: its workspace (and, where the ticks hand over, the
  // hand-off records) is allocated and its parameter block uploaded HERE, once, on the stream -- neither belongs inside the
  // capture below (an allocation is not capturable, and the parameters do not change between the ticks of a call).
  if (tick_plan.variant == 4) {
    const qmpc_status es = ensure_lane_buffers(h);
    if (es != QMPC_OK) return es;
    HIP_TRY(qmpc_lane_upload_params(h->lane_pslot, s, &h->dev, sizeof h->dev));
    if (tick_plan.iter_cap) (void)ensure_handoff_buffers(h);
  }
  if (warm) {                            // the cold first tick is not the tick the graph repeats
    const qmpc_status st = one_tick(true);
    if (st != QMPC_OK) return st;
    t_start = 1;
  }
  // (a stream the CALLER is capturing takes the ticks as plain launches, which become nodes of the caller's graph: no capture
  // is begun inside another)
  if (ticks - t_start > 1 && !stream_is_capturing(s) && hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
    const qmpc_status st = one_tick(false);
    const hipError_t ee = hipStreamEndCapture(s, &graph);
    if (st == QMPC_OK && ee == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess)
      captured = true;
    else
      (void)hipGetLastError();
  }
  qmpc_status rs = QMPC_OK;
  for (int t = t_start; t < ticks && rs == QMPC_OK; ++t) {
    if (captured) {
      if (hipGraphLaunch(exec, s) != hipSuccess) rs = QMPC_HIP_ERROR;
    } else {
      rs = one_tick(!warm);
    }
  }
  if (exec) {
    (void)hipStreamSynchronize(s);        // the executable graph must outlive its launches
    (void)hipGraphExecDestroy(exec);
  }
  if (graph) (void)hipGraphDestroy(graph);
  return rs;
}
}  // extern "C++"

// The closed loop's set-up on stream s: the trace row counter, reset to -1 stream-ordered (no host staging), and for a warm start
// in the per-tick form the handle's trajectory buffer, through which the solution travels from tick to tick (the persistent
// kernel keeps it in LDS; the first tick of a call starts cold)
// (the buffers alone: also what a call with ticks = 0 allocates on a handle that opted in to warm starts with controller records)
static qmpc_status ensure_loop_buffers(qmpc_handle* h, bool warm_ticks) {
  if (!h->d_loop_row) HIP_TRY(hipMalloc(&h->d_loop_row, sizeof(int)));
  if (warm_ticks && !h->d_traj_u)
    HIP_TRY(hipMalloc(&h->d_traj_u, sizeof(double) * 12 * (size_t)h->params.horizon * (size_t)h->max_batch));
  return QMPC_OK;
}
static qmpc_status loop_setup(qmpc_handle* h, hipStream_t s, bool warm_ticks) {
  const qmpc_status es = ensure_loop_buffers(h, warm_ticks);
  if (es != QMPC_OK) return es;
  // inside a stream capture of the caller's the reset is a kernel node like the ticks that follow it, not a memset node
  if (stream_is_capturing(s))
    HIP_TRY(qmpc_loop_row_reset_launch(s, h->d_loop_row));
  else
    HIP_TRY(hipMemsetAsync(h->d_loop_row, 0xFF, sizeof(int), s));
  return QMPC_OK;
}

// g != NULL: the joint-level kernel closes every tick (d_joint_pos in/out, d_cmd = the last tick's commands, d_trace_cmd
// one row per tick; either of the two may be NULL)
static qmpc_status loop_run_impl(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                 int32_t ticks, double* d_trace_forces, double* d_trace_contacts,
                                 const qmpc_leg_geometry* g, double* d_joint_pos, qmpc_joint_command* d_cmd,
                                 qmpc_joint_command* d_trace_cmd, void* stream) {
  if (!h || !lp || batch < 0 || ticks < 0 || (batch > 0 && !d_states)) return QMPC_BAD_ARGUMENT;
  if (g && batch > 0 && (!d_joint_pos || (!d_cmd && !d_trace_cmd))) return QMPC_BAD_ARGUMENT;
  if (h->params.model != QMPC_MODEL_QUAT && h->params.model != QMPC_MODEL_CONVEX) return QMPC_BAD_ARGUMENT;
  const bool convex = h->params.model == QMPC_MODEL_CONVEX;
  // the device tick of ConvexMpc carries the controller period as the literal 5 ms (velocity ramp, gait clock): a handle
  // with another knot spacing would silently part from the host class and the reference (ConvexMpc.cpp:9,62,208)
  if (convex && h->params.h != (float)(5.0 / 1000.0)) return QMPC_UNSUPPORTED;
  if (batch == 0 || ticks == 0) return QMPC_OK;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const bool warm = lp->warm_start != 0.0 && h->params.mode == QMPC_MODE_CONVERGED;
  const qmpc_status ss = loop_setup(h, s, warm);
  if (ss != QMPC_OK) return ss;
  const unsigned blocks = (unsigned)((batch + 63) / 64);
  const qmpc_loop_params LP = *lp;
  LegGeom G;
  std::memset(&G, 0, sizeof G);
  if (g) std::memcpy(&G, g, sizeof G);
  auto one_tick = [&](bool first) -> qmpc_status {
    if (convex)
      hipLaunchKernelGGL(qmpc_loop_front_convex_kernel, dim3(blocks), dim3(64), 0, s, LP, d_states,
                         reinterpret_cast<qmpc_convex_input*>(h->d_in), h->d_loop_row, (int)batch);
    else
      hipLaunchKernelGGL(qmpc_loop_front_kernel, dim3(blocks), dim3(64), 0, s, LP, d_states, h->d_in, h->d_loop_row, (int)batch);
    HIP_TRY(hipGetLastError());
    const qmpc_status st = loop_tick_solve(h, batch, s, warm, first, convex);
    if (st != QMPC_OK) return st;
    if (convex)
      hipLaunchKernelGGL(qmpc_loop_post_kernel<true>, dim3(blocks), dim3(64), 0, s, h->dev, LP, d_states, (const double*)h->d_forces,
                         (const qmpc_info*)h->d_info, d_trace_forces, d_trace_contacts, (const int*)h->d_loop_row, (int)batch);
    else
      hipLaunchKernelGGL(qmpc_loop_post_kernel<false>, dim3(blocks), dim3(64), 0, s, h->dev, LP, d_states, (const double*)h->d_forces,
                         (const qmpc_info*)h->d_info, d_trace_forces, d_trace_contacts, (const int*)h->d_loop_row, (int)batch);
    HIP_TRY(hipGetLastError());
    if (g) {
      hipLaunchKernelGGL(qmpc_loop_joint_kernel, dim3((unsigned)(((size_t)batch * 4 + 255) / 256)), dim3(256), 0, s, G,
                         (const qmpc_loop_state*)d_states, d_joint_pos, (qmpc_joint_feedback*)nullptr, d_cmd, d_trace_cmd,
                         (const int*)h->d_loop_row, (int)batch);
      HIP_TRY(hipGetLastError());
    }
    return QMPC_OK;
  };
  // the persistent kernel (ONE launch for all ticks) or the per-tick launch sequence below (qmpc_plan.h)
  const qmpc_plan lp_plan = plan(h->sel, batch, warm ? QMPC_CALL_WARM_LOOP : QMPC_CALL_LOOP, true, h->opts.handoff_failed);
  if (lp_plan.fused) {
    HIP_TRY(qmpc_fused_launch(lp_plan.variant, h->params.mode == QMPC_MODE_REFERENCE ? 1 : 0, convex ? 1 : 0, (int)batch, lp_plan.lds, s, &h->dev,
                              sizeof h->dev, &LP, d_states, h->d_in, h->d_forces, h->d_info, d_trace_forces, d_trace_contacts, (int)ticks,
                              lp_plan.gws ? h->d_gws : nullptr, g, d_joint_pos, d_cmd, d_trace_cmd));
    return QMPC_OK;
  }
  return replay_ticks(h, lp_plan, s, ticks, warm, one_tick);
}

qmpc_status qmpc_loop_run_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                 int32_t ticks, double* d_trace_forces, double* d_trace_contacts, void* stream) {
  return loop_run_impl(h, lp, batch, d_states, ticks, d_trace_forces, d_trace_contacts, nullptr, nullptr, nullptr, nullptr,
                       stream);
}

qmpc_status qmpc_loop_run_joint_device(qmpc_handle* h, const qmpc_loop_params* lp, const qmpc_leg_geometry* g, int32_t batch,
                                       qmpc_loop_state* d_states, double* d_joint_pos, int32_t ticks,
                                       qmpc_joint_command* d_cmd, qmpc_joint_command* d_trace_cmd, void* stream) {
  if (!g) return QMPC_BAD_ARGUMENT;
  return loop_run_impl(h, lp, batch, d_states, ticks, nullptr, nullptr, g, d_joint_pos, d_cmd, d_trace_cmd, stream);
}

static qmpc_status loop_records_host(int kind, qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                     int32_t ticks, const loop_recs& r);

qmpc_status qmpc_loop_run(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                          int32_t ticks, double* trace_forces, double* trace_contacts) {
  return loop_records_host(REC_PLAIN, h, lp, batch, states, ticks, loop_recs{nullptr, nullptr, trace_forces, trace_contacts});
}

// ---- the closed loop with per-robot controller and plant records (qmpc_loop_inst.hip) -------------------------------------
static_assert(sizeof(qmpc_plant_params) == 128, "qmpc_plant_params is 128 B");
int32_t qmpc_sizeof_plant_params(void) { return (int32_t)sizeof(qmpc_plant_params); }

void qmpc_plant_params_from(const qmpc_params* p, qmpc_plant_params* out) {
  if (!p || !out) return;
  std::memset(out, 0, sizeof *out);
  out->mass = p->mass;
  std::memcpy(out->inertia, p->inertia, sizeof out->inertia);
}

// the handle is ConvexMpc's and opted in to the loops with records (qmpc_set_convex_records): the kernels of qmpc_loop_crec.hip
static bool convex_records(const qmpc_handle* h) { return h->params.model == QMPC_MODEL_CONVEX && h->opts.convex_records; }

// the call-level checks of both entry points, for a call with at least one kind of record (QMPC_OK: go on)
static qmpc_status loop_instances_check(const qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, bool has_ctrl) {
  if (h->params.model != QMPC_MODEL_QUAT && h->params.model != QMPC_MODEL_CONVEX) return QMPC_BAD_ARGUMENT;
  // (a ConvexMpc handle: one that opted in only, qmpc_set_convex_records)
  const bool crec = convex_records(h);
  if ((h->params.model != QMPC_MODEL_QUAT && !crec) || h->params.mode != QMPC_MODE_CONVERGED) return QMPC_UNSUPPORTED;
  // (the device tick of ConvexMpc carries the controller period as the literal 5 ms: loop_run_impl)
  if (crec && h->params.h != (float)(5.0 / 1000.0)) return QMPC_UNSUPPORTED;
  // (controller records with the warm start: on a handle that opted in only -- QuatMpc: qmpc_set_loop_warm_records, ConvexMpc:
  // qmpc_set_convex_warm_records)
  if (has_ctrl && ((lp->warm_start != 0.0 && !(crec ? h->opts.convex_warm : h->opts.loop_warm_records)) || !h->sel.wform))
    return QMPC_UNSUPPORTED;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  // (the handle's policy refuses no call: a plan is NONE under QMPC_INSTANCES_AUTO exactly where it is under QMPC_INSTANCES_WAVE)
  if (batch > 0 && plan_loop_instances(h->sel, h->opts, batch, has_ctrl, lp->warm_start != 0.0).family == QMPC_KERNEL_NONE)
    return QMPC_UNSUPPORTED;
  return QMPC_OK;
}

// The buffers of a call with records, allocated before anything is launched or captured (a call with ticks = 0 stops after
// this): the per-instance and plant blocks and, where the ticks' solve is the lane kernel with per-lane parameters
// (QMPC_INSTANCES_AUTO), its workspace, sort scratch, parameter rows and hand-off records; for warm-started ticks with
// controller records the trajectory buffer the solution travels through.  *lpp: the call's plan -- re-planned without the
// hand-off where its records could not be allocated.
static qmpc_status loop_instances_buffers(qmpc_handle* h, int32_t batch, bool has_ctrl, bool warm, qmpc_plan* lpp) {
  qmpc_status es = ensure_instance_buffers(h);
  if (es == QMPC_OK) es = ensure_plant_buffers(h);
  if (es != QMPC_OK) return es;
  // (ConvexMpc: the scratch the outcome step of a call without outcome records runs on)
  if (convex_records(h) && !h->d_outcome) {
    HIP_TRY(hipMalloc(&h->d_outcome, sizeof(qmpc_loop_outcome) * (size_t)h->max_batch));
    // (its contents never reach a result -- the parameters that go with it halt no robot -- zeroed once all the same)
    HIP_TRY(hipMemsetAsync(h->d_outcome, 0, sizeof(qmpc_loop_outcome) * (size_t)h->max_batch, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  qmpc_plan p = plan_loop_instances(h->sel, h->opts, batch, has_ctrl, warm);
  if (has_ctrl && !p.fused && p.variant == 4) {
    es = ensure_lane_inst_buffers(h, false);
    if (es != QMPC_OK) return es;
    if (p.iter_cap && !ensure_handoff_buffers(h)) p = plan_loop_instances(h->sel, h->opts, batch, has_ctrl, warm);
  }
  if (has_ctrl && warm && !p.fused) {      // (an opted-in handle: what loop_setup would allocate after a ticks = 0 return)
    es = ensure_loop_buffers(h, true);
    if (es != QMPC_OK) return es;
  }
  if (lpp) *lpp = p;
  return QMPC_OK;
}

// The device-buffer closed loop of every kind, on the call's records as loop_recs_normalise left them (qmpc_loop_records.h: what
// is not NULL is part of the call).  REC_PLAIN without records is the plain loop.  Above it the kernels of the kind's unit run in
// place of the plain unit's; without ctrl and plant every robot's plant block carries the handle's mass and inverse inertia, and
// the call-level checks are those of a call with plant records.  Every record that is there is checked once after the plant
// expansion, in the order of the kinds: a robot whose record is refused is frozen through its plant block.  r.geom is a host
// pointer and travels as a kernel argument.
static qmpc_status loop_records_device(int kind, qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                       int32_t ticks, const loop_recs& recs, void* stream) {
  if (!h || !lp || batch < 0 || ticks < 0 || (batch > 0 && !d_states)) return QMPC_BAD_ARGUMENT;
  if (kind == REC_PLAIN && !recs.ctrl && !recs.plant)
    return loop_run_impl(h, lp, batch, d_states, ticks, recs.trace_forces, recs.trace_contacts, nullptr, nullptr, nullptr, nullptr, stream);
  const bool has_ctrl = recs.ctrl != nullptr;
  const qmpc_status cs = loop_instances_check(h, lp, batch, has_ctrl);
  if (cs != QMPC_OK || batch == 0) return cs;
  const bool warm = lp->warm_start != 0.0;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  qmpc_plan lpp;
  const qmpc_status es = loop_instances_buffers(h, batch, has_ctrl, warm, &lpp);
  if (es != QMPC_OK || ticks == 0) return es;      // ticks = 0: the buffers only (e.g. before the caller's stream capture)
  const qmpc_status ss = loop_setup(h, s, warm && !lpp.fused);
  if (ss != QMPC_OK) return ss;
  // the cold first tick of a warm-started call with controller records has a plan of its own (the lane form: no cap, no hand-off)
  const qmpc_plan lpp_first = (has_ctrl && warm && !lpp.fused) ? plan_loop_instances(h->sel, h->opts, batch, true, warm, /*first=*/true) : lpp;
  const qmpc_loop_params LP = *lp;
  // a ConvexMpc handle (opted in): one unit for the first three kinds -- a call without windows passes none (per_robot = 0), a
  // call without outcome records the handle's scratch and parameters that never halt a robot
  const bool crec = convex_records(h);
  const auto& R = kRec[kind][crec];
  loop_recs r = recs;
  qmpc_outcome_params op_none;
  std::memset(&op_none, 0, sizeof op_none);
  if (crec && kind == REC_PLAIN) {
    r.op = &op_none;
    r.outcomes = h->d_outcome;
  }
  // the records are expanded once per call: the controllers' blocks (or, for the persistent kernel without controller records,
  // the handle's block per robot) and the plant blocks with each robot's verdict
  if (has_ctrl) HIP_TRY(qmpc_wform_inst_expand_launch((int)batch, s, &h->dev, sizeof h->dev, r.ctrl, inst_dev(h), inst_status(h)));
  void* bcast = (!has_ctrl && lpp.fused) ? inst_dev(h) : nullptr;
  if (r.ctrl || r.plant)
    HIP_TRY(qmpc_loop_inst_expand_launch(s, &h->dev, sizeof h->dev, r.plant, r.ctrl, has_ctrl ? inst_status(h) : nullptr, bcast,
                                         plant_dev(h), (int)batch));
  else
    HIP_TRY(qmpc_loop_outcome_expand_base_launch(s, &h->dev, sizeof h->dev, bcast, plant_dev(h), (int)batch));
  if (r.push) HIP_TRY(qmpc_loop_push_check_launch(s, r.push, (int)r.per_robot, plant_dev(h), (int)batch));
  if (r.ground) HIP_TRY(qmpc_ground_tu::rec_ground_check_launch(s, r.ground, plant_dev(h), (int)batch));
  if (r.act) HIP_TRY(qmpc_act_tu::rec_act_check_launch(s, r.act, r.line, plant_dev(h), (int)batch));
  if (r.sense) HIP_TRY(qmpc_sense_tu::rec_sense_check_launch(s, r.sense, plant_dev(h), (int)batch));
  if (r.gait) HIP_TRY(qmpc_gait_tu::rec_gait_check_launch(s, r.gait, plant_dev(h), lp->dt, (int)batch));
  if (r.motor) HIP_TRY(qmpc_motor_tu::rec_motor_check_launch(s, r.motor, r.mtally, plant_dev(h), (int)batch));
  const rec_launch L = {s, inst_dev(h), plant_dev(h), &LP, d_states, h->d_in, h->d_forces, h->d_info, h->d_loop_row, (int)batch};
  if (lpp.fused) {
    HIP_TRY(R.fused_launch(lpp.variant, lpp.lds, (int)ticks, lpp.gws ? h->d_gws : nullptr, L, r));
    return QMPC_OK;
  }
  auto one_tick = [&](bool first) -> qmpc_status {
    HIP_TRY(R.front_launch(L, r));
    // with controller records the solve on the blocks expanded above (a warm-started call's solution travels through
    // h->d_traj_u), without them the plain loop's
    const qmpc_status st = !has_ctrl ? loop_tick_solve(h, batch, s, warm, first, crec)
                                     : inst_solve(h, first ? lpp_first : lpp, crec, !warm ? INST_TICK_COLD : first ? INST_TICK_FIRST : INST_TICK_WARM,
                                                  batch, h->d_in, h->d_forces, h->d_info, warm ? h->d_traj_u : nullptr, nullptr, s);
    if (st != QMPC_OK) return st;
    HIP_TRY(R.post_launch(L, r));
    return QMPC_OK;
  };
  // (the lane kernel's block in the table of the unit with per-lane parameters: once per call, outside the capture)
  if (has_ctrl && lpp.variant == 4)
    for (int w = 0; w <= (warm ? 1 : 0); ++w) HIP_TRY(kLaneInst[crec].start[w].upload_params(h->lane_pslot, s, &h->dev, sizeof h->dev));
  return replay_ticks(h, lpp, s, ticks, warm, one_tick);
}

// The host-buffer closed loop of every kind (qmpc_loop_run*), on the call's records as loop_recs_normalise left them: its checks,
// its buffers -- all allocated before the ticks = 0 return, which so prepares a later call of the same kind (the outcome call's
// ticks = 0 stops before h->d_outcome, as it always did; a call that stages windows or an optional record allocates it) -- and the
// staging, which only grows: states and traces through h->d_loop, [states | force trace | contact trace]; ctrl and plant to the
// staging halves of the per-instance and plant buffers, outcome records and windows to h->d_outcome and h->d_push, the optional
// records where kRecStage says.  Then the device-buffer call on the staged copies, and what it wrote comes back.
static qmpc_status loop_records_host(int kind, qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states,
                                     int32_t ticks, const loop_recs& r) {
  if (!h || !lp || batch < 0 || ticks < 0 || (batch > 0 && !states)) return QMPC_BAD_ARGUMENT;
  const size_t B = (size_t)batch, T = (size_t)ticks, MB = (size_t)h->max_batch;
  if (kind == REC_PLAIN && !r.ctrl && !r.plant) {      // the plain loop
    if (h->params.model != QMPC_MODEL_QUAT && h->params.model != QMPC_MODEL_CONVEX) return QMPC_BAD_ARGUMENT;
    if (batch == 0 || ticks == 0) return QMPC_OK;
    if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
    HIP_TRY(hipSetDevice(h->device));
  } else {
    const qmpc_status cs = loop_instances_check(h, lp, batch, r.ctrl != nullptr);
    if (cs != QMPC_OK || batch == 0) return cs;
    HIP_TRY(hipSetDevice(h->device));
    const qmpc_status es = loop_instances_buffers(h, batch, r.ctrl != nullptr, lp->warm_start != 0.0, nullptr);
    if (es != QMPC_OK) return es;
    if (r.push && h->push_cap < r.per_robot) {
      if (h->d_push) (void)hipFree(h->d_push);
      h->d_push = nullptr;
      h->push_cap = 0;
      HIP_TRY(hipMalloc(&h->d_push, sizeof(qmpc_push_params) * (size_t)r.per_robot * MB));
      h->push_cap = r.per_robot;
    }
    bool staged = r.push != nullptr;
    for (const rec_stage& s : kRecStage) staged = staged || s.get(r);
    if (staged && !h->d_outcome) HIP_TRY(hipMalloc(&h->d_outcome, sizeof(qmpc_loop_outcome) * MB));
    for (const rec_stage& s : kRecStage) {
      if (!s.get(r) || h->*s.buf) continue;
      size_t both = 0;      // the buffer holds max_batch of every record the table places in it
      for (const rec_stage& o : kRecStage) both += o.buf == s.buf ? o.elem : 0;
      HIP_TRY(hipMalloc(&(h->*s.buf), both * MB));
    }
    if (ticks == 0) return QMPC_OK;
    if (kind != REC_PLAIN && !h->d_outcome) HIP_TRY(hipMalloc(&h->d_outcome, sizeof(qmpc_loop_outcome) * MB));
  }
  const size_t n_st = (sizeof(qmpc_loop_state) / sizeof(double)) * B, n_tf = r.trace_forces ? 12 * B * T : 0,
               n_tc = r.trace_contacts ? 4 * B * T : 0;
  if (h->loop_cap < n_st + n_tf + n_tc) {
    if (h->d_loop) (void)hipFree(h->d_loop);
    h->d_loop = nullptr;
    h->loop_cap = 0;
    HIP_TRY(hipMalloc(&h->d_loop, sizeof(double) * (n_st + n_tf + n_tc)));
    h->loop_cap = n_st + n_tf + n_tc;
  }
  qmpc_loop_state* d_st = reinterpret_cast<qmpc_loop_state*>(h->d_loop);
  loop_recs d = r;      // the call on the staged copies: op and geom stay on the host
  d.trace_forces = r.trace_forces ? h->d_loop + n_st : nullptr;
  d.trace_contacts = r.trace_contacts ? h->d_loop + n_st + n_tf : nullptr;
  HIP_TRY(hipMemcpyAsync(d_st, states, sizeof(qmpc_loop_state) * B, hipMemcpyHostToDevice, h->stream));
  if (r.outcomes) HIP_TRY(hipMemcpyAsync(h->d_outcome, r.outcomes, sizeof(qmpc_loop_outcome) * B, hipMemcpyHostToDevice, h->stream));
  if (r.ctrl) HIP_TRY(hipMemcpyAsync(inst_rec(h), r.ctrl, sizeof(qmpc_instance_params) * B, hipMemcpyHostToDevice, h->stream));
  if (r.plant) HIP_TRY(hipMemcpyAsync(plant_rec(h), r.plant, sizeof(qmpc_plant_params) * B, hipMemcpyHostToDevice, h->stream));
  if (r.push) HIP_TRY(hipMemcpyAsync(h->d_push, r.push, sizeof(qmpc_push_params) * B * (size_t)r.per_robot, hipMemcpyHostToDevice, h->stream));
  d.outcomes = r.outcomes ? h->d_outcome : nullptr;
  d.ctrl = r.ctrl ? inst_rec(h) : nullptr;
  d.plant = r.plant ? plant_rec(h) : nullptr;
  d.push = r.push ? h->d_push : nullptr;
  for (const rec_stage& s : kRecStage) {
    if (!s.get(r)) continue;
    void* dst = static_cast<unsigned char*>(h->*s.buf) + s.before * MB;
    HIP_TRY(hipMemcpyAsync(dst, s.get(r), s.elem * B, hipMemcpyHostToDevice, h->stream));
    s.set(d, dst);
  }
  const qmpc_status rs = loop_records_device(kind, h, lp, batch, d_st, ticks, d, nullptr);
  if (rs != QMPC_OK) return rs;
  for (size_t i = sizeof kRecStage / sizeof kRecStage[0]; i-- > 0;) {
    const rec_stage& s = kRecStage[i];
    if (s.out && s.get(r)) HIP_TRY(hipMemcpyAsync(s.get(r), s.get(d), s.elem * B, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipMemcpyAsync(states, d_st, sizeof(qmpc_loop_state) * B, hipMemcpyDeviceToHost, h->stream));
  if (r.outcomes) HIP_TRY(hipMemcpyAsync(r.outcomes, h->d_outcome, sizeof(qmpc_loop_outcome) * B, hipMemcpyDeviceToHost, h->stream));
  if (d.trace_forces) HIP_TRY(hipMemcpyAsync(r.trace_forces, d.trace_forces, sizeof(double) * 12 * B * T, hipMemcpyDeviceToHost, h->stream));
  if (d.trace_contacts) HIP_TRY(hipMemcpyAsync(r.trace_contacts, d.trace_contacts, sizeof(double) * 4 * B * T, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return QMPC_OK;
}

// An entry point of kind `entry` with its caller's arguments r (what it does not take: NULL): the call they are
// (loop_recs_normalise: pointer checks only, before anything touches the handle) on the device-buffer path (device; stream) or the
// host-buffer path
static qmpc_status loop_records_call(bool device, int entry, qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch,
                                     qmpc_loop_state* states, int32_t ticks, loop_recs r, void* stream) {
  qmpc_leg_geometry go1;
  if (r.motor && !r.geom) qmpc_default_go1_geometry(&go1);
  int kind;
  if (loop_recs_normalise(entry, batch, &go1, &r, &kind) != QMPC_OK) return QMPC_BAD_ARGUMENT;
  return device ? loop_records_device(kind, h, lp, batch, states, ticks, r, stream) : loop_records_host(kind, h, lp, batch, states, ticks, r);
}

qmpc_status qmpc_loop_run_instances_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                           int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                           double* d_trace_forces, double* d_trace_contacts, void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts};
  return loop_records_call(true, REC_PLAIN, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_instances(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                    const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                    double* trace_contacts) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts};
  return loop_records_call(false, REC_PLAIN, h, lp, batch, states, ticks, r, nullptr);
}

// ---- the same closed loop with per-robot outcome records (qmpc_loop_outcome.hip) -------------------------------------------
static_assert(sizeof(qmpc_loop_outcome) == 128 && sizeof(qmpc_outcome_params) == 32, "qmpc_loop_outcome is 128 B, its parameters 4 doubles");
int32_t qmpc_sizeof_loop_outcome(void) { return (int32_t)sizeof(qmpc_loop_outcome); }

void qmpc_default_outcome_params(qmpc_outcome_params* op) {
  if (!op) return;
  std::memset(op, 0, sizeof *op);
  op->down_height = 0.15;
  op->down_upright = 0.5;
}

void qmpc_loop_outcome_init(qmpc_loop_outcome* o, int32_t batch) {
  if (!o) return;
  const double inf = std::numeric_limits<double>::infinity();
  for (int32_t i = 0; i < batch; ++i) {
    std::memset(&o[i], 0, sizeof o[i]);
    o[i].down_tick = -1.0;
    o[i].first_rejected_tick = -1.0;
    o[i].min_height = o[i].min_upright = inf;
    o[i].max_height_err = o[i].max_vel_err = o[i].max_ang_vel = o[i].max_force_z = o[i].iterations_max = -inf;
  }
}

qmpc_status qmpc_loop_run_outcomes_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                          int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                          double* d_trace_forces, double* d_trace_contacts, const qmpc_outcome_params* op,
                                          qmpc_loop_outcome* d_outcomes, void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts, op, d_outcomes};
  return loop_records_call(true, REC_OUTCOME, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_outcomes(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                   const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                   double* trace_contacts, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts, op, outcomes};
  return loop_records_call(false, REC_OUTCOME, h, lp, batch, states, ticks, r, nullptr);
}

// ---- the outcome loop under timed push windows per robot (qmpc_loop_push.hip) ------------------------------------------------
static_assert(sizeof(qmpc_push_params) == 64, "qmpc_push_params is 8 doubles");
int32_t qmpc_sizeof_push_params(void) { return (int32_t)sizeof(qmpc_push_params); }

qmpc_status qmpc_loop_run_pushes_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                        int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                        double* d_trace_forces, double* d_trace_contacts, const qmpc_outcome_params* op,
                                        qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                        void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts, op, d_outcomes, d_push, pushes_per_robot};
  return loop_records_call(true, REC_PUSH, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_pushes(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                 const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                 double* trace_contacts, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                                 const qmpc_push_params* push, int32_t pushes_per_robot) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts, op, outcomes, push, pushes_per_robot};
  return loop_records_call(false, REC_PUSH, h, lp, batch, states, ticks, r, nullptr);
}

// ---- the push loop on the robot's true ground: friction and normal-force limits per leg (qmpc_loop_ground.hip, qmpc_loop_cground.hip) ----
static_assert(sizeof(qmpc_ground_params) == 64 && sizeof(qmpc_ground_tally) == 32, "qmpc_ground_params is 8 doubles, qmpc_ground_tally 4");
int32_t qmpc_sizeof_ground_params(void) { return (int32_t)sizeof(qmpc_ground_params); }
int32_t qmpc_sizeof_ground_tally(void) { return (int32_t)sizeof(qmpc_ground_tally); }

void qmpc_ground_params_init(qmpc_ground_params* g, int32_t batch) {
  if (!g) return;
  const double inf = std::numeric_limits<double>::infinity();
  for (int32_t i = 0; i < batch; ++i)
    for (int l = 0; l < 4; ++l) g[i].mu[l] = g[i].fz_max[l] = inf;
}

void qmpc_ground_tally_init(qmpc_ground_tally* t, int32_t batch) {
  if (!t) return;
  for (int32_t i = 0; i < batch; ++i) {
    t[i].clipped_ticks = t[i].friction_leg_ticks = t[i].normal_leg_ticks = 0.0;
    t[i].first_clipped_tick = -1.0;
  }
}

qmpc_status qmpc_loop_run_ground_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                        int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                        double* d_trace_forces, double* d_trace_contacts, const qmpc_outcome_params* op,
                                        qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                        const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally, void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts, op, d_outcomes, d_push, pushes_per_robot, d_ground,
                       d_tally};
  return loop_records_call(true, REC_GROUND, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_ground(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                 const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                 double* trace_contacts, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                                 const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground,
                                 qmpc_ground_tally* tally) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts, op, outcomes, push, pushes_per_robot, ground, tally};
  return loop_records_call(false, REC_GROUND, h, lp, batch, states, ticks, r, nullptr);
}

// ---- the ground loop behind the robot's delay line and actuator lag (qmpc_loop_act.hip, qmpc_loop_cact.hip) ----------------------
static_assert(sizeof(qmpc_actuation_params) == 32 && sizeof(qmpc_actuation_line) == 896, "qmpc_actuation_params is 4 doubles, qmpc_actuation_line 112");
int32_t qmpc_sizeof_actuation_params(void) { return (int32_t)sizeof(qmpc_actuation_params); }
int32_t qmpc_sizeof_actuation_line(void) { return (int32_t)sizeof(qmpc_actuation_line); }

void qmpc_actuation_params_init(qmpc_actuation_params* act, int32_t batch) {
  if (!act) return;
  for (int32_t i = 0; i < batch; ++i) {
    act[i].delay_ticks = 0.0;
    act[i].alpha = 1.0;
    act[i].reserved[0] = act[i].reserved[1] = 0.0;
  }
}

void qmpc_actuation_line_init(qmpc_actuation_line* line, int32_t batch, const double* initial_forces_body) {
  if (!line) return;
  for (int32_t i = 0; i < batch; ++i) {
    for (int k = 0; k < 12; ++k) {
      const double f = initial_forces_body ? initial_forces_body[k] : 0.0;
      for (int c = 0; c < QMPC_MAX_DELAY; ++c) line[i].cmd[c][k] = f;
      line[i].applied[k] = f;
    }
    line[i].count = 0.0;
    line[i].reserved[0] = line[i].reserved[1] = line[i].reserved[2] = 0.0;
  }
}

qmpc_status qmpc_loop_run_actuation_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                           int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                           double* d_trace_forces, double* d_trace_contacts, const qmpc_outcome_params* op,
                                           qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                           const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                           const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line, void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts, op, d_outcomes, d_push, pushes_per_robot, d_ground,
                       d_tally, d_act, d_line};
  return loop_records_call(true, REC_ACT, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_actuation(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                    const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                    double* trace_contacts, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                                    const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground,
                                    qmpc_ground_tally* tally, const qmpc_actuation_params* act, qmpc_actuation_line* line) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts, op, outcomes, push, pushes_per_robot, ground, tally, act, line};
  return loop_records_call(false, REC_ACT, h, lp, batch, states, ticks, r, nullptr);
}

// ---- the actuation loop whose controller reads a measured state (qmpc_loop_sense.hip, qmpc_loop_csense.hip) -----------------------
static_assert(sizeof(qmpc_sense_params) == 256 && sizeof(qmpc_sense_seen) == 128, "qmpc_sense_params is 32 doubles, qmpc_sense_seen 16");
int32_t qmpc_sizeof_sense_params(void) { return (int32_t)sizeof(qmpc_sense_params); }
int32_t qmpc_sizeof_sense_seen(void) { return (int32_t)sizeof(qmpc_sense_seen); }

void qmpc_sense_params_init(qmpc_sense_params* sense, int32_t batch) {
  if (!sense) return;
  for (int32_t i = 0; i < batch; ++i) {
    for (int c = 0; c < 12; ++c) sense[i].bias[c] = sense[i].sigma[c] = 0.0;
    sense[i].seed = 0.0;
    for (int c = 0; c < 7; ++c) sense[i].reserved[c] = 0.0;
  }
}

void qmpc_sense_seen_init(qmpc_sense_seen* seen, int32_t batch) {
  if (!seen) return;
  for (int32_t i = 0; i < batch; ++i) {
    for (int c = 0; c < 13; ++c) seen[i].meas[c] = 0.0;
    seen[i].ticks = 0.0;
    seen[i].reserved[0] = seen[i].reserved[1] = 0.0;
  }
}

qmpc_status qmpc_loop_run_sensing_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                         int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                         double* d_trace_forces, double* d_trace_contacts, const qmpc_outcome_params* op,
                                         qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                         const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                         const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                                         const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen, void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts, op, d_outcomes, d_push, pushes_per_robot, d_ground,
                       d_tally, d_act, d_line, d_sense, d_seen};
  return loop_records_call(true, REC_SENSE, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_sensing(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                  const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                  double* trace_contacts, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                                  const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground,
                                  qmpc_ground_tally* tally, const qmpc_actuation_params* act, qmpc_actuation_line* line,
                                  const qmpc_sense_params* sense, qmpc_sense_seen* seen) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts, op, outcomes, push, pushes_per_robot, ground, tally, act, line,
                       sense, seen};
  return loop_records_call(false, REC_SENSE, h, lp, batch, states, ticks, r, nullptr);
}

// ---- the sensing loop in which every robot walks a gait of its own (qmpc_loop_gait.hip, qmpc_loop_cgait.hip) ---------------------
static_assert(sizeof(qmpc_gait_params) == 128, "qmpc_gait_params is 16 doubles");
int32_t qmpc_sizeof_gait_params(void) { return (int32_t)sizeof(qmpc_gait_params); }

void qmpc_default_gait_params(const qmpc_loop_params* lp, qmpc_gait_params* out) {
  if (!lp || !out) return;
  out->gait_freq = lp->gait_freq;
  for (int l = 0; l < 4; ++l) {
    out->first_stance[l] = (l == 0 || l == 3) ? 1.0 : 0.0;
    out->split[l] = 0.5;
    out->phase0[l] = 0.0;
  }
  for (int c = 0; c < 3; ++c) out->reserved[c] = 0.0;
}

void qmpc_loop_state_set_gait(qmpc_loop_state* s, const qmpc_gait_params* gait) {
  if (!s || !gait) return;
  for (int l = 0; l < 4; ++l) {
    qmpc_loop::loop_gait_reset(*gait, l, s->leg[l]);
    s->contacts[l] = s->leg[l].state;
  }
}

void qmpc_gait_predict(const qmpc_loop_params* lp, const qmpc_gait_params* g, const qmpc_loop_state* s, double h, int32_t N,
                       uint8_t* masks) {
  if (!s || !masks || (!g && !lp)) return;
  qmpc_gait_params trot;
  if (!g) qmpc_default_gait_params(lp, &trot);      // the reference's trot at lp->gait_freq, the identity record
  qmpc_loop::loop_gait_predict(g ? *g : trot, *s, h, (int)N, masks);
}

qmpc_status qmpc_loop_run_gaits_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                       int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                       double* d_trace_forces, double* d_trace_contacts, const qmpc_outcome_params* op,
                                       qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                       const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                       const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                                       const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen, const qmpc_gait_params* d_gait,
                                       void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts, op, d_outcomes, d_push, pushes_per_robot, d_ground,
                       d_tally, d_act, d_line, d_sense, d_seen, d_gait};
  return loop_records_call(true, REC_GAIT, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_gaits(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                double* trace_contacts, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                                const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground,
                                qmpc_ground_tally* tally, const qmpc_actuation_params* act, qmpc_actuation_line* line,
                                const qmpc_sense_params* sense, qmpc_sense_seen* seen, const qmpc_gait_params* gait) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts, op, outcomes, push, pushes_per_robot, ground, tally, act, line,
                       sense, seen, gait};
  return loop_records_call(false, REC_GAIT, h, lp, batch, states, ticks, r, nullptr);
}

// ---- the gait loop whose delivered foot force respects the motors' torque limits (qmpc_loop_motor.hip, qmpc_loop_cmotor.hip) --------
static_assert(sizeof(qmpc_motor_params) == 128, "qmpc_motor_params is 16 doubles");
static_assert(sizeof(qmpc_motor_tally) == 320, "qmpc_motor_tally is 40 doubles");
int32_t qmpc_sizeof_motor_params(void) { return (int32_t)sizeof(qmpc_motor_params); }
int32_t qmpc_sizeof_motor_tally(void) { return (int32_t)sizeof(qmpc_motor_tally); }

void qmpc_default_motor_params(qmpc_motor_params* out) {
  if (!out) return;
  for (int a = 0; a < 12; ++a) out->tau_max[a] = HUGE_VAL;
  for (int a = 0; a < 4; ++a) out->reserved[a] = 0.0;
}

void qmpc_motor_tally_init(qmpc_motor_tally* out) {
  if (!out) return;
  std::memset(out, 0, sizeof *out);
  qmpc_loop_joint_init(out->joint_pos, 1);
  out->first_clipped_tick = -1.0;
}

qmpc_status qmpc_loop_run_motors_device(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* d_states,
                                        int32_t ticks, const qmpc_instance_params* d_ctrl, const qmpc_plant_params* d_plant,
                                        double* d_trace_forces, double* d_trace_contacts, const qmpc_outcome_params* op,
                                        qmpc_loop_outcome* d_outcomes, const qmpc_push_params* d_push, int32_t pushes_per_robot,
                                        const qmpc_ground_params* d_ground, qmpc_ground_tally* d_tally,
                                        const qmpc_actuation_params* d_act, qmpc_actuation_line* d_line,
                                        const qmpc_sense_params* d_sense, qmpc_sense_seen* d_seen, const qmpc_gait_params* d_gait,
                                        const qmpc_leg_geometry* geom, const qmpc_motor_params* d_motor,
                                        qmpc_motor_tally* d_motor_tally, void* stream) {
  const loop_recs r = {d_ctrl, d_plant, d_trace_forces, d_trace_contacts, op, d_outcomes, d_push, pushes_per_robot, d_ground,
                       d_tally, d_act, d_line, d_sense, d_seen, d_gait, geom, d_motor, d_motor_tally};
  return loop_records_call(true, REC_MOTOR, h, lp, batch, d_states, ticks, r, stream);
}

qmpc_status qmpc_loop_run_motors(qmpc_handle* h, const qmpc_loop_params* lp, int32_t batch, qmpc_loop_state* states, int32_t ticks,
                                 const qmpc_instance_params* ctrl, const qmpc_plant_params* plant, double* trace_forces,
                                 double* trace_contacts, const qmpc_outcome_params* op, qmpc_loop_outcome* outcomes,
                                 const qmpc_push_params* push, int32_t pushes_per_robot, const qmpc_ground_params* ground,
                                 qmpc_ground_tally* tally, const qmpc_actuation_params* act, qmpc_actuation_line* line,
                                 const qmpc_sense_params* sense, qmpc_sense_seen* seen, const qmpc_gait_params* gait,
                                 const qmpc_leg_geometry* geom, const qmpc_motor_params* motor, qmpc_motor_tally* motor_tally) {
  const loop_recs r = {ctrl, plant, trace_forces, trace_contacts, op, outcomes, push, pushes_per_robot, ground, tally, act, line,
                       sense, seen, gait, geom, motor, motor_tally};
  return loop_records_call(false, REC_MOTOR, h, lp, batch, states, ticks, r, nullptr);
}

// Diagnostic: per-instance phase cycle counts (s_memtime) of one solve launch.
// cycles_out: [batch][16] int64 on the host; slots 0..14 follow the PH_* enum of qmpc_kernels.hip (setup, expansions,
// operand build, MFMA + stage terms, stage solve, cost-to-go update, directions, rollout, misc, rotation pre-pass,
// rollout gain / broadcast / step, apply, MFMA drain); slot 15 = iterations.
qmpc_status qmpc_debug_profile(qmpc_handle* h, int32_t batch, const qmpc_input* in, int64_t* cycles_out) {
  if (!h || batch < 1 || !in || !cycles_out) return QMPC_BAD_ARGUMENT;
  if (h->params.model != QMPC_MODEL_QUAT || h->params.mode != QMPC_MODE_CONVERGED) return QMPC_BAD_ARGUMENT;
  if (batch > h->max_batch) return QMPC_BATCH_TOO_LARGE;
  HIP_TRY(hipSetDevice(h->device));
  long long* d_prof = nullptr;
  HIP_TRY(hipMalloc(&d_prof, sizeof(long long) * 16 * (size_t)batch));
  HIP_TRY(hipMemsetAsync(d_prof, 0, sizeof(long long) * 16 * (size_t)batch, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_in, in, sizeof(qmpc_input) * (size_t)batch, hipMemcpyHostToDevice, h->stream));
  const qmpc_plan p = plan(h->sel, batch, QMPC_CALL_PROFILE, true, h->opts.handoff_failed);
  if (p.variant >= 3) {
    HIP_TRY(qmpc_wform_launch(QMPC_MODEL_QUAT, 0, p.variant, 1, (int)batch, p.lds, h->stream, &h->dev, sizeof h->dev, h->d_in, h->d_forces, h->d_info,
                              nullptr, nullptr, d_prof, p.gws ? h->d_gws : nullptr));
  } else {
    const int k = dense_solve_slot(QMPC_MODEL_QUAT, p.variant, true);
    if (k < 0) HIP_TRY(hipErrorInvalidValue);
    hipLaunchKernelGGL(kDenseSolve[k], dim3((unsigned)batch), dim3(kWave), p.lds, h->stream, h->dev, h->d_in, h->d_forces, h->d_info,
                       (double*)nullptr, (double*)nullptr, (int)batch, d_prof, p.gws ? h->d_gws : nullptr);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(cycles_out, d_prof, sizeof(long long) * 16 * (size_t)batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipFree(d_prof));
  return QMPC_OK;
}

// Diagnostic (not part of the drop-in surface): C = X' * Y on [12][16] tiles via
// the FP64 MFMA path; host buffers of 192 doubles each.
qmpc_status qmpc_selftest_mtm(int32_t device, const double* X, const double* Y, double* Cout) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device >= ndev) return QMPC_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  double* d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof(double) * 3 * MAT));
  HIP_TRY(hipMemcpy(d, X, sizeof(double) * MAT, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d + MAT, Y, sizeof(double) * MAT, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(qmpc_selftest_kernel, dim3(1), dim3(kWave), 0, 0, d, d + MAT, d + 2 * MAT);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(Cout, d + 2 * MAT, sizeof(double) * MAT, hipMemcpyDeviceToHost));
  HIP_TRY(hipFree(d));
  return QMPC_OK;
}

// Diagnostic: cross-lane primitives on 64 doubles; out holds 9 x 64 doubles
// (row-group broadcasts 0..3, wave sum/max/min, row_newbcast:5, quad_perm[1,1,1,1]).
qmpc_status qmpc_selftest_lanes(int32_t device, const double* in, double* out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device >= ndev) return QMPC_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  double* d = nullptr;
  HIP_TRY(hipMalloc(&d, sizeof(double) * 64 * 10));
  HIP_TRY(hipMemcpy(d, in, sizeof(double) * 64, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(qmpc_selftest_lanes_kernel, dim3(1), dim3(kWave), 0, 0, d, d + 64);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d + 64, sizeof(double) * 64 * 9, hipMemcpyDeviceToHost));
  HIP_TRY(hipFree(d));
  return QMPC_OK;
}

}  // extern "C"
