// hrgym_host_batch.h -- the batch handle of the C ABI (include/hrgym.h: hrg_batch_*, hrg_debug_*): the variant table that picks a batch's kernels, the task table that
// says what a task is, create as its named steps, destroy, reset / check / step, the accessors, the scripted experts and demonstration datasets attached to a batch, and the test taps of the base unit's
// kernels.  Included by the base unit only (hrgym_hip.hip), behind hrgym_host.h.

struct TaskTraits;
struct hrg_batch {
  int device = 0;
  int32_t n_envs = 0;
  int64_t env_id0 = 0;
  DeviceMem mem;                       // behind every d_ pointer below
  DevModel* d_model = nullptr;
  double* d_frames = nullptr;
  double* d_pose = nullptr;            // per-frame human pose table (DevModel::pose_tab): the tasks whose kernels read it (TaskTraits::pose_table)
  size_t pose_bytes = 0;
  double* d_hull = nullptr;            // hull vertices of the arm links (robot_hulls)
  bool hulls = false;                  // a hull variant steps this batch: of the ReachHuman kernels (hrgym_hulls.hip), the cube kernels (hrgym_box_hulls.hip) or a task's own (hrgym_*_hulls.hip)
  unsigned long long* d_mpr_fallback = nullptr;   // hull - cube pairs whose MPR did not converge (DevModel::mpr_fallback; hrg_batch_mpr_fallbacks)
  hrg_env_state* d_states = nullptr;
  double* d_rcaps = nullptr;
  double* d_hcaps = nullptr;
  int32_t* d_nh = nullptr;
  float* d_scratch_obs = nullptr;
  hrg_box_state* d_boxes = nullptr;   // the manipulation object of each env (PickPlaceHumanCart)
  hrg_stack_state* d_stacks = nullptr; // the four cubes of each env (CollaborativeStackingCart)
  hrg_hammer_state* d_hammers = nullptr; // board, hammer, nail of each env (CollaborativeHammeringCart)
  int32_t* d_order = nullptr;          // launch order of the step kernel (StepOrder): two orders of n_envs + two pairs of counters
  int32_t parity = 0;                  // which of the two orders the next step launch reads
  const TaskTraits* traits = nullptr;  // the row of the batch's task (HRG_TASKS)
  bool ik = false;                     // the Cartesian action front-end is on: action rows are [dx, dy, dz, gripper, -, -, -]
  bool has_expert = false;             // hrg_batch_expert_attach
  hrg_expert_desc expert;              // the attached expert (a kernel argument of the two expert kernels)
  ExpertBuffers ex;
  std::unique_ptr<DeviceMem> ex_mem;   // behind every pointer of `ex`; replaced by an attach
  bool has_dataset = false;            // hrg_batch_dataset_attach
  hrg_dataset_desc dataset;            // the attached dataset's parameters (a kernel argument of the two dataset kernels; its host pointers are nulled)
  DatasetDev ds;
  std::unique_ptr<DeviceMem> ds_mem;   // behind every pointer of `ds`; replaced by an attach
  bool timing = false;
  bool taps = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;     // a pair is in exactly one of the two lists
  ~hrg_batch() {
    for (const auto* list : {&events, &pool})
      for (const auto& p : *list) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
  }
};

// the progress table of the level-waves priority (StepOrder.fair): one per device, shared by the batches and kernel variants that run on it; never freed
static int32_t* fair_table(int device) {
  static int32_t* tab[64] = {nullptr};
  if (device < 0 || device >= 64) return nullptr;
  if (!tab[device]) {
    int32_t* p = nullptr;
    if (hipMalloc(&p, sizeof(int32_t) * HRG_FAIR_SLOTS) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, sizeof(int32_t) * HRG_FAIR_SLOTS) != hipSuccess) { hipFree(p); return nullptr; }
    tab[device] = p;
  }
  return tab[device];
}

// Every kernel variant of the library, once: X(family, hulls, name suffix).  The suffix is the one HRG_SYM gives the variant's translation unit (hrgym_device.h);
// a line here, the wrapper .hip that sets its flags and its entry in _lib.SOURCES are what a new variant needs.
enum { HRG_FAM_REACH, HRG_FAM_BOX, HRG_FAM_HO, HRG_FAM_LIFT, HRG_FAM_STACK, HRG_FAM_HAMMER, HRG_NFAMILY };
#define HRG_VARIANTS(X)                                              \
  X(HRG_FAM_REACH, 0, )          X(HRG_FAM_REACH, 1, _hull)          \
  X(HRG_FAM_BOX, 0, _box)        X(HRG_FAM_BOX, 1, _box_hull)        \
  X(HRG_FAM_HO, 0, _ho)          X(HRG_FAM_HO, 1, _ho_hull)          \
  X(HRG_FAM_LIFT, 0, _lift)      X(HRG_FAM_LIFT, 1, _lift_hull)      \
  X(HRG_FAM_STACK, 0, _stack)    X(HRG_FAM_STACK, 1, _stack_hull)    \
  X(HRG_FAM_HAMMER, 0, _hammer)  X(HRG_FAM_HAMMER, 1, _hammer_hull)
#define X(family, hulls, sfx)                                                                  \
  extern "C" __attribute__((visibility("hidden"))) hrg_launch_step_fn hrg_launch_step##sfx;    \
  extern "C" __attribute__((visibility("hidden"))) hrg_launch_reset_fn hrg_launch_reset##sfx;  \
  extern "C" __attribute__((visibility("hidden"))) hrg_launch_chain_fk_fn hrg_launch_chain_fk##sfx;  \
  extern "C" __attribute__((visibility("hidden"))) hrg_launch_self_pairs_fn hrg_launch_self_pairs##sfx;  \
  extern "C" __attribute__((visibility("hidden"))) hrg_launch_narrowphase_fn hrg_launch_narrowphase##sfx;
HRG_VARIANTS(X)
#undef X
struct Variant { hrg_launch_step_fn* step; hrg_launch_reset_fn* reset; hrg_launch_chain_fk_fn* chain_fk; hrg_launch_self_pairs_fn* self_pairs; hrg_launch_narrowphase_fn* narrowphase; };
struct VariantTable { Variant v[HRG_NFAMILY][2]; };   // [family][hulls]
static constexpr VariantTable make_variants() {
  VariantTable t{};
#define X(family, hulls, sfx) t.v[family][hulls] = Variant{hrg_launch_step##sfx, hrg_launch_reset##sfx, hrg_launch_chain_fk##sfx, hrg_launch_self_pairs##sfx, hrg_launch_narrowphase##sfx};
  HRG_VARIANTS(X)
#undef X
  return t;
}
static const VariantTable g_variants = make_variants();

// Every task of the library, once: what the host has to know about an HRG_TASK_* beyond the values of its descriptor.  A row here, its row in the Python package's
// tasks.py and whatever is new in the kernel and the descriptor are what a new task of an existing family needs.
enum { HRG_OBJ_NONE, HRG_OBJ_BOXES, HRG_OBJ_STACKS, HRG_OBJ_HAMMERS };   // the per-env object block a task's kernels stream: none, d_boxes, d_stacks, d_hammers
struct TaskTraits {
  int task, family, objs;   // HRG_TASK_*, HRG_FAM_*, HRG_OBJ_*
  bool pose_table;          // its kernels are built with HRG_POSE_TABLE; every other task steps with a cube kernel or a hand-mocap kernel, which keep the live tree kinematics
  bool dataset;             // a dataset or snapshot can hold its state: (hrg_env_state, hrg_box_state) is all of it
  unsigned experts, sirs;   // bit k: HRG_EXPERT_k / HRG_SIR_k reads the observation of this task (HRG_SIR_NONE fits every task that a dataset can hold)
};
#define E(x) (1u << HRG_EXPERT_##x)
#define S(x) (1u << HRG_SIR_##x)
static constexpr TaskTraits HRG_TASKS[] = {
  {HRG_TASK_REACH, HRG_FAM_REACH, HRG_OBJ_NONE, true, true, E(REACH), S(REACH)},                    // hrgym_hip.hip, hrgym_hulls.hip
  {HRG_TASK_PICK_PLACE, HRG_FAM_BOX, HRG_OBJ_BOXES, false, true, E(PICK_PLACE), S(PICK_PLACE)},      // PP-AIR; (also PickPlaceCloseHumanCart)
  {HRG_TASK_INSPECTION, HRG_FAM_BOX, HRG_OBJ_BOXES, false, true, 0, 0},
  {HRG_TASK_POINTING, HRG_FAM_BOX, HRG_OBJ_BOXES, false, true, 0, 0},
  // the handover tasks: HRH-AIR, RHH-AIR; the pick-place state reward serves "any environment that can be solved using the PickPlaceHumanCartExpert"
  {HRG_TASK_HANDOVER_H2R, HRG_FAM_HO, HRG_OBJ_BOXES, false, true, E(PICK_PLACE), S(PICK_PLACE)},
  {HRG_TASK_HANDOVER_R2H, HRG_FAM_HO, HRG_OBJ_BOXES, false, true, E(PICK_PLACE), S(PICK_PLACE)},
  {HRG_TASK_LIFTING, HRG_FAM_LIFT, HRG_OBJ_BOXES, true, true, E(LIFTING), S(LIFTING)},               // hrgym_lift.hip: the board is its box
  {HRG_TASK_STACKING, HRG_FAM_STACK, HRG_OBJ_STACKS, false, false, E(PICK_PLACE), 0},                // CS-AIR; its state lives in a further array (d_stacks)
  // ReachHuman with its box: no expert and no state reward, the cube kernel serves object_quat in the goal_difference columns
  {HRG_TASK_REACH_BOX, HRG_FAM_BOX, HRG_OBJ_BOXES, false, true, 0, 0},
  {HRG_TASK_HAMMERING, HRG_FAM_HAMMER, HRG_OBJ_HAMMERS, false, false, E(HAMMERING), 0},              // its state lives in a further array (d_hammers)
  {HRG_TASK_REACH_CART, HRG_FAM_BOX, HRG_OBJ_BOXES, false, true, E(REACH_CART), S(REACH)},           // the Reach state reward: three goal_difference columns, the other three zero
};
#undef E
#undef S
static const TaskTraits* task_traits(int task) {   // null: no such task
  for (const TaskTraits& t : HRG_TASKS)
    if (t.task == task) return &t;
  return nullptr;
}
// what hrg_batch_get_ / set_ of an object block answer on a batch whose task streams another one, by HRG_OBJ_* (null: every batch has the array)
static const char* const g_objs_missing[] = {nullptr, nullptr, "not a CollaborativeStackingCart batch", "not a CollaborativeHammeringCart batch"};

// the variant that steps a batch, and the object array its kernels stream (null: the ReachHuman kernels stream none)
static const Variant& batch_variant(const hrg_batch* b, void** objs) {
  const TaskTraits& t = *b->traits;
  *objs = t.objs == HRG_OBJ_BOXES ? (void*)b->d_boxes : t.objs == HRG_OBJ_STACKS ? (void*)b->d_stacks : t.objs == HRG_OBJ_HAMMERS ? (void*)b->d_hammers : nullptr;
  return g_variants.v[t.family][b->hulls ? 1 : 0];
}

// one env's block of a per-env device array <-> the host (hrg_batch_get_ / set_ state, box, stack, hammer); objs = the HRG_OBJ_* the array belongs to: a batch of
// a task with another block has no such array (g_objs_missing)
template <class T>
static int env_block_copy(hrg_batch* b, int32_t env, T* hrg_batch::*arr, void* buf_host, size_t bytes, bool get, int objs) {
  if (!b || env < 0 || env >= b->n_envs || bytes != sizeof(T)) return fail(HRG_ERR_INVALID, "bad env index or buffer size");
  if (g_objs_missing[objs] && b->traits->objs != objs) return fail(HRG_ERR_INVALID, g_objs_missing[objs]);
  T* const dev = b->*arr;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  if (get) HIPCHK(hipMemcpy(buf_host, dev + env, bytes, hipMemcpyDeviceToHost));
  else HIPCHK(hipMemcpy(dev + env, buf_host, bytes, hipMemcpyHostToDevice));
  return HRG_OK;
}

static void mat_from_quat(double* M, const double* q) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  M[0] = 1 - 2 * (y * y + z * z); M[1] = 2 * (x * y - w * z); M[2] = 2 * (x * z + w * y);
  M[3] = 2 * (x * y + w * z); M[4] = 1 - 2 * (x * x + z * z); M[5] = 2 * (y * z - w * x);
  M[6] = 2 * (x * z - w * y); M[7] = 2 * (y * z + w * x); M[8] = 1 - 2 * (x * x + y * y);
}

extern "C" {

const char* hrg_version(void) { return "hrgym-hip 0.1.0 (gfx950)"; }
size_t hrg_state_bytes(void) { return sizeof(hrg_env_state); }
size_t hrg_box_bytes(void) { return sizeof(hrg_box_state); }
size_t hrg_stack_bytes(void) { return sizeof(hrg_stack_state); }
size_t hrg_hammer_bytes(void) { return sizeof(hrg_hammer_state); }

// hrg_batch_create in four steps.  The first: what a descriptor and its clip table must satisfy, before anything touches the device.
static int batch_check(const hrg_model_desc* desc, const hrg_clip_table* clips) {
  if (desc->failsafe_sdot != 0.0) return fail(HRG_ERR_INVALID, "failsafe_sdot must be 0: SSM / OFF brake to a stop, PFL computes its speed from pfl_v_safe / pfl_reach");
  if (desc->shield_type == HRG_SHIELD_PFL) {
    if (!(desc->pfl_v_safe > 0)) return fail(HRG_ERR_INVALID, "PFL: pfl_v_safe must be positive");
    for (int j = 0; j < NARM; j++) if (!(desc->pfl_reach[j] > 0)) return fail(HRG_ERR_INVALID, "PFL: pfl_reach must be positive");
  }
  for (int i = 0; i < NARM; i++)   // mj_Euler's implicit damping treats the arm's joint damping as a perturbation (euler_robot_tree): one Neumann term, error (h d / M)^2
    if (!(desc->jnt_damping[i] >= 0 && desc->timestep * desc->jnt_damping[i] * desc->dof_invweight0[i] < 1e-3))
      return fail(HRG_ERR_UNSUPPORTED, "arm joint damping too large for the implicit-damping expansion (h d / M must stay below 1e-3; robot.xml: 1e-4)");
  if ((desc->jnt_damping[NARM] > 0) != (desc->jnt_damping[NARM + 1] > 0)) return fail(HRG_ERR_UNSUPPORTED, "the two finger slides must both carry damping, or neither");
  if (desc->solimp[4] != 2.0) return fail(HRG_ERR_UNSUPPORTED, "solimp power must be 2 (MuJoCo's default): the HIP stepper evaluates the impedance sigmoid as a square");
  if (clips->n_clips < 1 || clips->n_clips > HRG_MAX_CLIPS || clips->n_clips != desc->n_clips) return fail(HRG_ERR_INVALID, "clip table / desc.n_clips mismatch");
  for (int i = 0; i < NV; i++) {
    if ((i < NARM) != (desc->jnt_type[i] == 0)) return fail(HRG_ERR_INVALID, "expected 6 hinges followed by 2 slides");
    if (i < NARM && desc->body_parent[i] != i - 1) return fail(HRG_ERR_INVALID, "arm must be a serial chain");
    if (i < NARM && !(desc->jnt_axis[i][0] == 0 && desc->jnt_axis[i][1] == 0 && desc->jnt_axis[i][2] == 1)) return fail(HRG_ERR_INVALID, "arm hinges must turn about the local z axis");
    if (i >= NARM && desc->body_parent[i] != NARM - 1) return fail(HRG_ERR_INVALID, "fingers must hang off the last link");
  }
  for (int c = 0; c < HRG_NSHIELD_RCAP; c++)
    if (desc->scap_body[c] != (c < NARM ? c : NARM - 1)) return fail(HRG_ERR_INVALID, "shield capsule c must sit on link c (gripper on link 6)");
  if (desc->n_bodypart > HRG_NBODYPART_MAX || desc->n_extremity > HRG_NEXTREMITY_MAX) return fail(HRG_ERR_INVALID, "too many body parts");
  const TaskTraits* const t = task_traits(desc->task);
  if (!t) return fail(HRG_ERR_UNSUPPORTED, "unknown task");
  if (desc->task == HRG_TASK_STACKING) {
    if (!(desc->box_inertia[0] == desc->box_inertia[1] && desc->box_inertia[1] == desc->box_inertia[2]))
      return fail(HRG_ERR_UNSUPPORTED, "CollaborativeStackingCart: the HIP stepper stacks cubes (object_full_size with three equal edges)");
    for (int c = 0; c < clips->n_clips; c++) {
      const int32_t* kf = clips->clip_stack_keyframes[c];
      if (!(kf[0] >= 0 && kf[0] <= kf[1] && kf[1] <= kf[2] && kf[2] <= kf[3] && kf[3] <= kf[4] && clips->clip_n_loop[c] >= 0 && clips->clip_n_loop[c] <= HRG_MAX_LOOP &&
            clips->clip_n_loop2[c] >= 0 && clips->clip_n_loop2[c] <= HRG_MAX_LOOP))
        return fail(HRG_ERR_INVALID, "CollaborativeStackingCart: every clip needs five ascending keyframes and at most 4 loop sines per waiting phase in its info");
    }
  }
  if (desc->task == HRG_TASK_LIFTING && !(desc->min_balance > -1 && desc->min_balance < 1)) return fail(HRG_ERR_INVALID, "CollaborativeLiftingCart: min_balance must lie in (-1, 1)");
  if (HRG_IS_HANDOVER(desc->task))
    for (int c = 0; c < clips->n_clips; c++)
      if (!(clips->clip_n_loop2[c] >= 0 && clips->clip_n_loop2[c] <= HRG_MAX_LOOP)) return fail(HRG_ERR_INVALID, "HumanRobotHandoverCart: at most 4 loop sines per stage");
  if (desc->task == HRG_TASK_INSPECTION || HRG_IS_HANDOVER(desc->task))
    for (int c = 0; c < clips->n_clips; c++)
      if (!(clips->clip_n_loop[c] >= 0 && clips->clip_n_loop[c] <= HRG_MAX_LOOP && clips->clip_keyframes[c][0] >= 0 && clips->clip_keyframes[c][0] <= clips->clip_keyframes[c][1]))
        return fail(HRG_ERR_INVALID, "HumanObjectInspectionCart: every clip needs keyframes (k0 <= k1) and at most 4 loop sines in its info");
  if (desc->ik_enabled && !(desc->ik_max_iter >= 1 && desc->ik_max_iter <= 1000 && desc->ik_damping > 0 && desc->ik_action_limit > 0 && desc->ik_residual_threshold >= 0))
    return fail(HRG_ERR_INVALID, "ik: need 1 <= max_iter <= 1000, damping > 0, action_limit > 0, residual_threshold >= 0");
  if (desc->task == HRG_TASK_HAMMERING) {
    if (!(desc->hm_board_mass > 0 && desc->hm_hammer_mass > 0 && desc->hm_nail_mass > 0 && desc->hm_nail_range > 0 && desc->hm_nail_invweight > 0 && desc->n_obj_placements > 0 &&
          desc->hm_board_inertia[0] > 0 && desc->hm_board_inertia[1] > 0 && desc->hm_board_inertia[2] > 0 && desc->hm_hammer_inertia[0] > 0 && desc->hm_hammer_inertia[1] > 0 &&
          desc->hm_hammer_inertia[2] > 0))
      return fail(HRG_ERR_INVALID, "CollaborativeHammeringCart needs positive board / hammer / nail masses and inertias, a nail range and n_obj_placements > 0");
    for (int c = 0; c < clips->n_clips; c++)
      if (!(clips->clip_keyframes[c][0] >= 0 && clips->clip_keyframes[c][0] <= clips->clip_keyframes[c][1] && clips->clip_n_loop[c] >= 0 && clips->clip_n_loop[c] <= HRG_MAX_LOOP))
        return fail(HRG_ERR_INVALID, "CollaborativeHammeringCart: every clip needs two ascending keyframes and at most 4 loop sines in its info");
  } else   // a box block, or the stack: its four cubes share box_half / box_mass / box_inertia
  if (t->objs != HRG_OBJ_NONE && !(desc->box_half[0] > 0 && desc->box_half[1] > 0 && desc->box_half[2] > 0 && desc->box_mass > 0 && desc->box_inertia[0] > 0 && desc->box_inertia[1] > 0 &&
                                     desc->box_inertia[2] > 0 && desc->box_inertia_mean > 0 && desc->box_invweight_rot > 0 && desc->n_targets > 0 && desc->n_obj_placements > 0))
    return fail(HRG_ERR_INVALID, "PickPlaceHumanCart needs box_half, box_mass, box_inertia, n_targets, n_obj_placements > 0");
  int maxd = 0;
  for (int i = 0; i < HRG_NHB; i++) maxd = desc->hb_depth[i] > maxd ? desc->hb_depth[i] : maxd;
  if (maxd + 1 > 16) return fail(HRG_ERR_INVALID, "human tree deeper than 15");
  int n_in_pos = 0;
  for (int k = 0; k < desc->n_bodypart; k++) {
    if (desc->bp_joint[k][0] < 0 || desc->bp_joint[k][0] >= HRG_NHJ || desc->bp_joint[k][1] < 0 || desc->bp_joint[k][1] >= HRG_NHJ) return fail(HRG_ERR_INVALID, "body part joint outside the human's sites");
    n_in_pos += desc->bp_in_pos[k] ? 1 : 0;
  }
  for (int k = 0; k < desc->n_extremity; k++)
    if (desc->ext_joint[k] < 0 || desc->ext_joint[k] >= HRG_NHJ) return fail(HRG_ERR_INVALID, "extremity joint outside the human's sites");
  if (2 * desc->n_bodypart + desc->n_extremity + n_in_pos > HRG_NHCAP_MAX) return fail(HRG_ERR_INVALID, "more than 64 human reach capsules");   // (the records batch_fill_model writes)
  int64_t tot = 0;
  for (int c = 0; c < clips->n_clips; c++) {
    if (clips->clip_len[c] < 1 || clips->clip_offset[c] != tot) return fail(HRG_ERR_INVALID, "clip table must be densely packed");
    tot += clips->clip_len[c];
  }
  if (tot != clips->total_frames) return fail(HRG_ERR_INVALID, "clip table total_frames mismatch");
  for (int c = 0; c < HRG_NRCAP; c++)   // (the kernels index the tree kinematics in LDS with it: DevModel::rcap_lane)
    if (desc->rcap_body[c] < -1 || desc->rcap_body[c] >= NV) return fail(HRG_ERR_INVALID, "rcap_body: a robot capsule rides on the base (-1) or on a body of the tree");
  if (desc->robot_hulls) {
    if (!g_variants.v[t->family][1].step)   // HRG_VARIANTS has no [family][1] line (today every family has one)
      return fail(HRG_ERR_UNSUPPORTED, "robot_hulls: no hull variant of the step kernel for this task");
    if (!desc->hull_verts || desc->hull_off[0] != 0) return fail(HRG_ERR_INVALID, "robot_hulls: hull_verts / hull_off missing");
    for (int h = 0; h < HRG_NHULL; h++)
      if (!(desc->hull_off[h + 1] > desc->hull_off[h] + 3 && desc->hull_off[h + 1] <= 1000000)) return fail(HRG_ERR_INVALID, "robot_hulls: every hull needs at least four vertices");
  }
  return HRG_OK;
}

// The second: the host's DevModel of a checked descriptor, every entry but the four device pointers (batch_upload sets them).  The device reads these bytes.
static void batch_fill_model(const hrg_model_desc* desc, const hrg_clip_table* clips, DevModel* hm) {
  memset(hm, 0, sizeof *hm);
  hm->m = *desc;
  mat_from_quat(hm->Rbase, desc->base_quat);
  for (int i = 0; i < NV; i++) {
    mat_from_quat(hm->Rq[i], desc->body_quat[i]);
    int mask = 0;
    for (int k = i; k >= 0; k = desc->body_parent[k]) mask |= 1 << k;
    hm->anc_mask[i] = mask;
  }
  int maxd = 0;
  for (int i = 0; i < HRG_NHB; i++) maxd = desc->hb_depth[i] > maxd ? desc->hb_depth[i] : maxd;
  hm->hb_maxdepth = maxd;
  { // mj_makeImpedance constants of solref (the oracle's `impedance`)
    double tc = desc->solref[0];
    const double dr = desc->solref[1], dmax = desc->solimp[1];
    if (tc < 2 * desc->timestep) tc = 2 * desc->timestep;
    hm->sol_K = 1.0 / (dmax * dmax * tc * tc * dr * dr);
    hm->sol_Bd = 2.0 / (dmax * tc);
  }
  for (int c = 0; c < HRG_NRCAP; c++) {
    double d2 = 0;
    for (int a = 0; a < 3; a++) d2 += (desc->rcap_p2[c][a] - desc->rcap_p1[c][a]) * (desc->rcap_p2[c][a] - desc->rcap_p1[c][a]);
    hm->rcap_hl[c] = 0.5 * sqrt(d2);
  }
  for (int c = 0; c < HRG_NHB; c++) {
    double d2 = 0;
    for (int a = 0; a < 3; a++) d2 += (desc->hcap_p2[c][a] - desc->hcap_p1[c][a]) * (desc->hcap_p2[c][a] - desc->hcap_p1[c][a]);
    hm->hcap_hl[c] = 0.5 * sqrt(d2);
  }
  for (int i = 0; i < HRG_NHB; i++) hm->hb_jump[0][i] = desc->hb_parent[i];
  for (int s = 1; s < 4; s++)
    for (int i = 0; i < HRG_NHB; i++) { const int a = hm->hb_jump[s - 1][i]; hm->hb_jump[s][i] = a < 0 ? -1 : hm->hb_jump[s - 1][a]; }
  hm->hb_njump = 0;
  while ((1 << hm->hb_njump) < maxd + 1) hm->hb_njump++;
  int n = 0;
  // (kind, joints, thickness, v_max, a_max or ball length) of reach capsule n as the record the shield's lanes load
  auto hc_set = [&](int n, int kind, int j1, int j2, double th, double v, double al) { hm->hc[n].th = th; hm->hc[n].v = v; hm->hc[n].al = al; hm->hc[n].kj = kind | (j1 << 8) | (j2 << 16); hm->hc[n].pad = 0; };
  for (int k = 0; k < desc->n_bodypart; k++, n++) hc_set(n, 0, desc->bp_joint[k][0], desc->bp_joint[k][1], desc->bp_thickness[k], desc->bp_vmax[k], desc->bp_amax[k]);
  for (int k = 0; k < desc->n_bodypart; k++, n++) hc_set(n, 1, desc->bp_joint[k][0], desc->bp_joint[k][1], desc->bp_thickness[k], desc->bp_vmax[k], 0.0);
  for (int k = 0; k < desc->n_extremity; k++, n++) hc_set(n, 2, desc->ext_joint[k], desc->ext_joint[k], desc->ext_thickness[k], desc->ext_vmax[k], desc->ext_length[k]);
  for (int k = 0; k < desc->n_bodypart; k++)
    if (desc->bp_in_pos[k]) hc_set(n++, 3, desc->bp_joint[k][0], desc->bp_joint[k][1], desc->bp_thickness[k], desc->bp_vmax[k], 0.0);
  hm->hc_n = n;
  int ns = 0;
  for (int i = 0; i < HRG_NRCAP; i++)
    for (int j = i + 1; j < HRG_NRCAP; j++)
      if ((desc->rcap_selfmask[i] >> j) & 1u) {
        // the longer capsule of the pair is the cull's segment (s), the other one its sphere (o): collide, self_near
        double len2[2];
        for (int e = 0; e < 2; e++) {
          const int c = e ? j : i;
          len2[e] = 0;
          for (int a = 0; a < 3; a++) len2[e] += (desc->rcap_p2[c][a] - desc->rcap_p1[c][a]) * (desc->rcap_p2[c][a] - desc->rcap_p1[c][a]);
        }
        const bool seg_j = len2[1] > len2[0];
        const int s = seg_j ? j : i, o = seg_j ? i : j;
        DevModel::SelfRec& r = hm->self_rec[ns++];
        r.ij = i | (j << 8) | (s << 16) | (o << 24);
        r.body_j = desc->rcap_body[j];
        r.inv_len2 = len2[seg_j] <= 1e-12 ? 0.0 : 1.0 / len2[seg_j];
        r.bound = hm->rcap_hl[o] + desc->rcap_r[i] + desc->rcap_r[j] + 1e-9;
        r.r_j = desc->rcap_r[j];
      }
  hm->n_self = ns;
  for (int l = 0; l < 6 * HRG_NRCAP; l++) {   // robot_capsules_world's lanes (v[0] of a base capsule: hrg_model_constants_kernel)
    const int c = l / 6, e = (l % 6) / 3, a = l % 3, bd = desc->rcap_body[c];
    DevModel::RcapLane& r = hm->rcap_lane[l];
    for (int q = 0; q < 3; q++) r.v[q] = e ? desc->rcap_p2[c][q] : desc->rcap_p1[c][q];
    r.k = bd < 0 ? -1 : 3 * bd + a;
  }
  int nc = 0;
  for (int i = 0; i < 8; i++)
    for (int j = i + 1; j < 8; j++)
      if (((desc->chk_selfmask[i] >> j) & 1u) && nc < 32) { hm->chk_i[nc] = i; hm->chk_j[nc] = j; nc++; }
  hm->n_chk = nc;
  hm->phase_mask = 0xff;
  {
    double se, ve, ae;
    path_plan(&hm->brake_full, 0.0, 1.0, 0.0, desc->failsafe_sdot, desc->path_amax, desc->path_jmax);
    hm->brake_T = path_total(&hm->brake_full);
    path_eval(&hm->brake_full, hm->brake_T, desc->failsafe_sdot, &se, &ve, &ae);
    hm->brake_ds = se;
  }
#ifdef HRG_STAMPS
  if (const char* pm = getenv("HRG_PHASE_MASK")) hm->phase_mask = atoi(pm); // diagnostic build only: results are invalid
#endif
  hm->clips = *clips;
  if (desc->robot_hulls) hull_centroids(desc->hull_verts, desc->hull_off, hm->hull_cen);
}

// The third: the clip frames, the hull vertices and the model on the device, and the two kernels that finish the model there.
static int batch_upload(hrg_batch* b, const hrg_model_desc* desc, const hrg_clip_table* clips, DevModel* hm) {
  DeviceMem& m = b->mem;
  const size_t frames = (size_t)clips->total_frames;
  bool ok = m.upload(b->d_frames, clips->frames, HRG_FRAME_DIM * frames);
  if (ok && b->traits->pose_table) {   // filled by hrg_pose_table_kernel once the model is on the device
    b->pose_bytes = sizeof(double) * HRG_POSE_DIM * frames;
    ok = m.zeros(b->d_pose, HRG_POSE_DIM * frames);
  }
  if (ok && desc->robot_hulls)   // convex hulls of the arm links: the vertex table goes to device memory like the clip frames
    ok = m.upload(b->d_hull, desc->hull_verts, 3 * (size_t)desc->hull_off[HRG_NHULL]) && m.zeros(b->d_mpr_fallback, 1);
  hm->clips.frames = b->d_frames;
  hm->pose_tab = b->d_pose;
  hm->hull_dev = b->d_hull;
  hm->mpr_fallback = b->d_mpr_fallback;
  if (!ok || !m.upload(b->d_model, hm, 1)) return nomem("batch", m);
  hipLaunchKernelGGL(hrg_model_constants_kernel, dim3(1), dim3(64), 0, 0, b->d_model);   // fric_*, eul_*, rcap_mid, rcap_lane of the base: in the device's own arithmetic
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  if (b->d_pose) {
    hipLaunchKernelGGL(hrg_pose_table_kernel, dim3((unsigned)clips->total_frames), dim3(64), 0, 0, b->d_model, b->d_pose);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
  }
  return HRG_OK;
}

// The fourth: the per-env arrays.  No env has an episode yet, and both launch orders are the identity.
static int batch_env_arrays(hrg_batch* b) {
  const size_t n = (size_t)b->n_envs;
  std::vector<hrg_env_state> init(n);
  memset(init.data(), 0, sizeof(hrg_env_state) * n);
  for (auto& s : init) s.episode = -1;
  std::vector<int32_t> ord(2 * n + 4, 0);
  for (size_t e = 0; e < n; e++) ord[e] = ord[n + e] = (int32_t)e;
  DeviceMem& m = b->mem;
  if (!(m.upload(b->d_states, init.data(), n) && m.zeros(b->d_rcaps, 7 * HRG_NSHIELD_RCAP * n) && m.zeros(b->d_hcaps, 7 * HRG_NHCAP_MAX * n) && m.zeros(b->d_nh, n) &&
        m.zeros(b->d_scratch_obs, HRG_OBS_DIM * n) && m.zeros(b->d_boxes, n) && (b->traits->objs != HRG_OBJ_HAMMERS || m.zeros(b->d_hammers, n)) &&
        (b->traits->objs != HRG_OBJ_STACKS || m.zeros(b->d_stacks, n)) && m.upload(b->d_order, ord.data(), ord.size())))
    return nomem("batch", m);
  HIPCHK(hipDeviceSynchronize());
  return HRG_OK;
}

int hrg_batch_create(const hrg_model_desc* desc, const hrg_clip_table* clips, int32_t n_envs, int64_t env_id0, int32_t device, hrg_batch** out) {
  if (!desc || !clips || !out || n_envs <= 0) return fail(HRG_ERR_INVALID, "null argument or n_envs <= 0");
  if (int rc = batch_check(desc, clips)) return rc;
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_batch> b(new hrg_batch());
  b->device = device; b->n_envs = n_envs; b->env_id0 = env_id0; b->traits = task_traits(desc->task); b->ik = desc->ik_enabled != 0; b->hulls = desc->robot_hulls != 0;
  std::unique_ptr<DevModel> hm(new DevModel());
  batch_fill_model(desc, clips, hm.get());
  if (int rc = batch_upload(b.get(), desc, clips, hm.get())) return rc;
  if (int rc = batch_env_arrays(b.get())) return rc;
  *out = b.release();
  return HRG_OK;
}

void hrg_batch_destroy(hrg_batch* b) { destroy_handle(b); }

int hrg_batch_reset(hrg_batch* b, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!b) return fail(HRG_ERR_INVALID, "null batch");
  HIPCHK(hipSetDevice(b->device));
  void* objs;
  const Variant& v = batch_variant(b, &objs);
  v.reset(b->n_envs, (hipStream_t)stream, b->d_model, b->d_states, mask_dev, obs_dev, b->env_id0, objs);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

int hrg_batch_check_actions(hrg_batch* b, const double* actions_dev, uint8_t* collides_dev, void* stream) {
  if (!b || !actions_dev || !collides_dev) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(hrg_check_kernel, HRG_LAUNCH_DIMS(b->n_envs), 0, (hipStream_t)stream, b->d_model, b->d_states, actions_dev, collides_dev, b->n_envs);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

int hrg_batch_step(hrg_batch* b, double* actions_dev, float* obs_dev, float* term_obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* info_dev, void* stream) {
  if (!b || !actions_dev || !obs_dev || !reward_dev || !done_dev || !info_dev) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = (hipStream_t)stream;
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (b->timing) {
    if (!b->pool.empty()) { ev = b->pool.back(); b->pool.pop_back(); }
    else { HIPCHK(hipEventCreate(&ev.first)); HIPCHK(hipEventCreate(&ev.second)); }
    HIPCHK(hipEventRecord(ev.first, st));
  }
  int32_t* fair = fair_table(b->device);
  if (!fair) return fail(HRG_ERR_HIP, "cannot allocate the wave-progress table");
  const StepOrder ord{b->d_order, b->n_envs, b->parity, fair};
  void* objs;
  const Variant& v = batch_variant(b, &objs);
  v.step(b->n_envs, st, b->d_model, b->d_states, actions_dev, obs_dev, term_obs_dev, reward_dev, done_dev, info_dev, b->taps ? b->d_rcaps : nullptr, b->taps ? b->d_hcaps : nullptr,
         b->taps ? b->d_nh : nullptr, b->env_id0, b->d_scratch_obs, objs, ord);
  HIPCHK(hipGetLastError());
  b->parity ^= 1;
  if (b->timing) { HIPCHK(hipEventRecord(ev.second, st)); b->events.push_back(ev); }
  return HRG_OK;
}

int hrg_batch_launch_order(hrg_batch* b, int32_t* order_host, int32_t* n_busy_host) {
  if (!b || !order_host || !n_busy_host) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  const size_t n = (size_t)b->n_envs;
  HIPCHK(hipMemcpy(order_host, b->d_order + (size_t)b->parity * n, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(n_busy_host, b->d_order + 2 * n + 2 * (size_t)b->parity, sizeof(int32_t), hipMemcpyDeviceToHost));   // the front counter that filled this order
  return HRG_OK;
}

int hrg_batch_contacts(hrg_batch* b, int32_t* pairs_host, int32_t* ncon_host) {
  if (!b) return fail(HRG_ERR_INVALID, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  std::vector<hrg_env_state> st((size_t)b->n_envs);
  HIPCHK(hipMemcpy(st.data(), b->d_states, sizeof(hrg_env_state) * (size_t)b->n_envs, hipMemcpyDeviceToHost));
  for (int e = 0; e < b->n_envs; e++) {
    ncon_host[e] = st[e].ncon;
    memcpy(pairs_host + (size_t)e * HRG_NCON_MAX * 2, st[e].con_pairs, sizeof(int32_t) * HRG_NCON_MAX * 2);
  }
  return HRG_OK;
}

int hrg_batch_capsules(hrg_batch* b, double* robot_host, double* human_host, int32_t* n_human_host) {
  if (!b) return fail(HRG_ERR_INVALID, "null batch");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(robot_host, b->d_rcaps, sizeof(double) * 7 * HRG_NSHIELD_RCAP * (size_t)b->n_envs, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(human_host, b->d_hcaps, sizeof(double) * 7 * HRG_NHCAP_MAX * (size_t)b->n_envs, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(n_human_host, b->d_nh, sizeof(int32_t) * (size_t)b->n_envs, hipMemcpyDeviceToHost));
  return HRG_OK;
}

int hrg_batch_get_state(hrg_batch* b, int32_t env, void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_states, buf_host, bytes, true, HRG_OBJ_NONE); }
int hrg_batch_set_state(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_states, (void*)buf_host, bytes, false, HRG_OBJ_NONE); }
int hrg_batch_get_box(hrg_batch* b, int32_t env, void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_boxes, buf_host, bytes, true, HRG_OBJ_BOXES); }
int hrg_batch_set_box(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_boxes, (void*)buf_host, bytes, false, HRG_OBJ_BOXES); }
int hrg_batch_get_stack(hrg_batch* b, int32_t env, void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_stacks, buf_host, bytes, true, HRG_OBJ_STACKS); }
int hrg_batch_set_stack(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_stacks, (void*)buf_host, bytes, false, HRG_OBJ_STACKS); }
int hrg_batch_get_hammer(hrg_batch* b, int32_t env, void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_hammers, buf_host, bytes, true, HRG_OBJ_HAMMERS); }
int hrg_batch_set_hammer(hrg_batch* b, int32_t env, const void* buf_host, size_t bytes) { return env_block_copy(b, env, &hrg_batch::d_hammers, (void*)buf_host, bytes, false, HRG_OBJ_HAMMERS); }

int hrg_batch_get_states(hrg_batch* b, const int32_t* envs_host, int32_t n, void* states_host, void* boxes_host) {
  if (!b || !envs_host || !states_host || n < 0) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  for (int32_t k = 0; k < n; k++) {
    const int32_t e = envs_host[k];
    if (e < 0 || e >= b->n_envs) return fail(HRG_ERR_INVALID, "bad env index");
    HIPCHK(hipMemcpyAsync((hrg_env_state*)states_host + k, b->d_states + e, sizeof(hrg_env_state), hipMemcpyDeviceToHost, 0));
    if (boxes_host) HIPCHK(hipMemcpyAsync((hrg_box_state*)boxes_host + k, b->d_boxes + e, sizeof(hrg_box_state), hipMemcpyDeviceToHost, 0));
  }
  HIPCHK(hipDeviceSynchronize());
  return HRG_OK;
}

int hrg_batch_set_states(hrg_batch* b, const int32_t* envs_host, int32_t n, const void* states_host, const void* boxes_host) {
  if (!b || !envs_host || !states_host || n < 0) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  for (int32_t k = 0; k < n; k++) {
    const int32_t e = envs_host[k];
    if (e < 0 || e >= b->n_envs) return fail(HRG_ERR_INVALID, "bad env index");
    HIPCHK(hipMemcpyAsync(b->d_states + e, (const hrg_env_state*)states_host + k, sizeof(hrg_env_state), hipMemcpyHostToDevice, 0));
    if (boxes_host) HIPCHK(hipMemcpyAsync(b->d_boxes + e, (const hrg_box_state*)boxes_host + k, sizeof(hrg_box_state), hipMemcpyHostToDevice, 0));
  }
  HIPCHK(hipDeviceSynchronize());
  return HRG_OK;
}

int hrg_batch_mpr_fallbacks(hrg_batch* b, int64_t* count_host) {
  if (!b || !count_host) return fail(HRG_ERR_INVALID, "null argument");
  *count_host = 0;
  if (!b->d_mpr_fallback) return HRG_OK;   // no hulls: no MPR
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  unsigned long long c = 0;
  HIPCHK(hipMemcpy(&c, b->d_mpr_fallback, sizeof c, hipMemcpyDeviceToHost));
  *count_host = (int64_t)c;
  return HRG_OK;
}

int hrg_batch_enable_taps(hrg_batch* b, int32_t on) {
  if (!b) return fail(HRG_ERR_INVALID, "null batch");
  b->taps = on != 0;
  return HRG_OK;
}

// the time between the events of the first pairs of b->events, summed: `n` counts the pairs read
static int event_times(hrg_batch* b, double& tot, size_t& n) {
  for (tot = 0, n = 0; n < b->events.size(); n++) {
    const auto& p = b->events[n];
    HIPCHK(hipEventSynchronize(p.second));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
    tot += ms;
  }
  return HRG_OK;
}

int hrg_batch_kernel_time(hrg_batch* b, double* avg_ms, int64_t* n_launches) {
  if (!b) return fail(HRG_ERR_INVALID, "null batch");
  HIPCHK(hipSetDevice(b->device));
  double tot;
  size_t n;
  const int rc = event_times(b, tot, n);
  b->pool.insert(b->pool.end(), b->events.begin(), b->events.begin() + n);   // the pairs read move to the pool, on either path
  b->events.erase(b->events.begin(), b->events.begin() + n);
  if (rc != HRG_OK) return rc;
  b->timing = true; // first call arms the timer
  if (avg_ms) *avg_ms = n ? tot / (double)n : 0.0;
  if (n_launches) *n_launches = n;
  return HRG_OK;
}

int hrg_batch_pose_table_bytes(hrg_batch* b, int64_t* bytes_host) {
  if (!b || !bytes_host) return fail(HRG_ERR_INVALID, "null argument");
  *bytes_host = (int64_t)b->pose_bytes;
  return HRG_OK;
}

// ---- scripted experts + action-based imitation reward (csrc/hrgym_expert.h) ----
int hrg_batch_expert_attach(hrg_batch* b, const hrg_expert_desc* desc) {
  if (!b || !desc) return fail(HRG_ERR_INVALID, "null argument");
  b->has_expert = false;   // until the descriptor has passed and every buffer below exists and is zeroed: a refused attach leaves no expert attached
  if (desc->expert < HRG_EXPERT_REACH || desc->expert > HRG_EXPERT_REACH_CART) return fail(HRG_ERR_UNSUPPORTED, "unknown expert");
  if (!(b->traits->experts >> desc->expert & 1u)) return fail(HRG_ERR_UNSUPPORTED, "this expert does not read the observation of the batch's task");
  if ((desc->cartesian != 0) != (desc->expert != HRG_EXPERT_REACH)) return fail(HRG_ERR_UNSUPPORTED, "ReachHumanExpert acts in joint space, every other expert in Cartesian space");
  if ((desc->cartesian != 0) != b->ik) return fail(HRG_ERR_UNSUPPORTED, "the expert's action form is not the batch's (Cartesian experts need the IK front-end, ik_enabled)");
  const int width = desc->cartesian ? 4 : HRG_ACT_DIM;
  for (int k = 0; k < width; k++)
    if (!(desc->act_low[k] < desc->act_high[k])) return fail(HRG_ERR_INVALID, "expert: action bounds need low < high");
  if (!(desc->signal_to_noise_ratio >= 0 && desc->signal_to_noise_ratio <= 1 && desc->delta_time >= 0)) return fail(HRG_ERR_INVALID, "expert: need 0 <= signal_to_noise_ratio <= 1 and delta_time >= 0");
  if (desc->reward_enabled) {
    if (!(desc->iota_m > 0 && desc->iota_g > 0)) return fail(HRG_ERR_INVALID, "imitation reward: iota_m and iota_g must be positive");
    if (!(desc->alpha >= 0 && desc->alpha <= 1 && desc->beta >= 0 && desc->beta <= 1)) return fail(HRG_ERR_INVALID, "imitation reward: alpha and beta must lie in [0, 1]");
    for (int fn : {desc->m_sim_fn, desc->g_sim_fn})
      if (fn != HRG_SIM_GAUSSIAN && fn != HRG_SIM_TANH) return fail(HRG_ERR_INVALID, "imitation reward: unknown similarity function");
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  const size_t n = (size_t)b->n_envs;
  ExpertBuffers& x = b->ex;
  b->ex_mem.reset();
  x = ExpertBuffers{};
  b->ex_mem.reset(new DeviceMem());
  DeviceMem& m = *b->ex_mem;
  if (!(m.zeros(x.act, HRG_ACT_DIM * n) && m.zeros(x.sim, 2 * n) && m.zeros(x.ou_y, HRG_ACT_DIM * n) && m.zeros(x.ou_calls, n) && m.zeros(x.acc, 3 * n))) return nomem("expert", m);
  HIPCHK(hipDeviceSynchronize());
  b->expert = *desc;
  b->has_expert = true;
  return HRG_OK;
}

int hrg_batch_expert_actions(hrg_batch* b, const float* obs_dev, double* actions_out_dev, void* stream) {
  if (!b || !obs_dev || !actions_out_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!b->has_expert) return fail(HRG_ERR_INVALID, "no expert attached (hrg_batch_expert_attach)");
  HIPCHK(hipSetDevice(b->device));
  hipLaunchKernelGGL(hrg_expert_pre_kernel, dim3((unsigned)((b->n_envs + HRG_EXPERT_BLOCK - 1) / HRG_EXPERT_BLOCK)), dim3(HRG_EXPERT_BLOCK), 0, (hipStream_t)stream, b->expert, obs_dev,
                     (const double*)nullptr, actions_out_dev, (double*)nullptr, b->ex.ou_y, b->ex.ou_calls, b->env_id0, b->n_envs);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

int hrg_batch_step_imitation(hrg_batch* b, double* actions_dev, float* obs_dev, float* term_obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* info_dev, float* imit_dev,
                             void* stream) {
  if (!b || !actions_dev || !obs_dev || !reward_dev || !done_dev || !info_dev || !imit_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!b->has_expert) return fail(HRG_ERR_INVALID, "no expert attached (hrg_batch_expert_attach)");
  if (!b->expert.reward_enabled) return fail(HRG_ERR_INVALID, "the expert was attached without an imitation reward (reward_enabled = 0)");
  HIPCHK(hipSetDevice(b->device));
  const dim3 grid((unsigned)((b->n_envs + HRG_EXPERT_BLOCK - 1) / HRG_EXPERT_BLOCK)), block(HRG_EXPERT_BLOCK);
  hipLaunchKernelGGL(hrg_expert_pre_kernel, grid, block, 0, (hipStream_t)stream, b->expert, (const float*)obs_dev, (const double*)actions_dev, b->ex.act, b->ex.sim, b->ex.ou_y,
                     b->ex.ou_calls, b->env_id0, b->n_envs);
  HIPCHK(hipGetLastError());
  const int rc = hrg_batch_step(b, actions_dev, obs_dev, term_obs_dev, reward_dev, done_dev, info_dev, stream);
  if (rc != HRG_OK) return rc;
  hipLaunchKernelGGL(hrg_imitation_post_kernel, grid, block, 0, (hipStream_t)stream, b->expert, (const double*)b->ex.sim, (const uint8_t*)done_dev, reward_dev, b->ex.acc, imit_dev,
                     b->n_envs);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

// ---- demonstration datasets: reference state initialisation + state-based imitation reward (csrc/hrgym_dataset.h) ----
int hrg_batch_snapshot(hrg_batch* b, void* states_out_dev, void* boxes_out_dev, void* stream) {
  if (!b || !states_out_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!b->traits->dataset) return fail(HRG_ERR_UNSUPPORTED, "snapshot: the stacking and hammering tasks keep their state in further arrays");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpyAsync(states_out_dev, b->d_states, sizeof(hrg_env_state) * (size_t)b->n_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (boxes_out_dev && b->traits->objs == HRG_OBJ_BOXES)
    HIPCHK(hipMemcpyAsync(boxes_out_dev, b->d_boxes, sizeof(hrg_box_state) * (size_t)b->n_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return HRG_OK;
}

int hrg_batch_dataset_attach(hrg_batch* b, const hrg_dataset_desc* desc) {
  if (!b || !desc) return fail(HRG_ERR_INVALID, "null argument");
  b->has_dataset = false;   // until the descriptor has passed and every buffer below exists: a refused attach leaves no dataset attached
  if (!b->traits->dataset) return fail(HRG_ERR_UNSUPPORTED, "dataset: the stacking and hammering tasks keep their state in further arrays, which a dataset does not hold");
  if (desc->sir_kind < HRG_SIR_NONE || desc->sir_kind > HRG_SIR_LIFTING) return fail(HRG_ERR_UNSUPPORTED, "unknown sir_kind");
  if (desc->sir_kind != HRG_SIR_NONE && !(b->traits->sirs >> desc->sir_kind & 1u)) return fail(HRG_ERR_UNSUPPORTED, "this state imitation reward does not read the observation of the batch's task");
  if (!desc->ep_offset || !desc->states || !desc->obs || desc->n_episodes <= 0) return fail(HRG_ERR_INVALID, "dataset: null array or no episode");
  if ((desc->boxes != nullptr) != (b->traits->objs == HRG_OBJ_BOXES)) return fail(HRG_ERR_INVALID, "dataset: a box array is needed exactly when the batch's task has a box block");
  if (desc->ep_offset[0] != 0 || desc->ep_offset[desc->n_episodes] != desc->total_T) return fail(HRG_ERR_INVALID, "dataset: ep_offset must run from 0 to total_T");
  for (int64_t k = 0; k < desc->n_episodes; k++) {
    const int64_t T = desc->ep_offset[k + 1] - desc->ep_offset[k];
    if (T <= 0) return fail(HRG_ERR_INVALID, "dataset: an episode without a transition (T = 0)");
    if (T > INT32_MAX) return fail(HRG_ERR_INVALID, "dataset: episode too long");
  }
  if (desc->n_episodes > INT32_MAX) return fail(HRG_ERR_INVALID, "dataset: too many episodes");
  if (!(desc->rsi_prob >= 0 && desc->rsi_prob <= 1)) return fail(HRG_ERR_INVALID, "dataset: rsi_prob must lie in [0, 1]");
  if (desc->sir_kind != HRG_SIR_NONE) {
    if (!(desc->iota_m > 0 && desc->iota_g > 0)) return fail(HRG_ERR_INVALID, "state imitation reward: iota_m and iota_g must be positive");
    if (!(desc->alpha >= 0 && desc->alpha <= 1 && desc->beta >= 0 && desc->beta <= 1)) return fail(HRG_ERR_INVALID, "state imitation reward: alpha and beta must lie in [0, 1]");
    if (!(desc->et_dist >= 0)) return fail(HRG_ERR_INVALID, "state imitation reward: et_dist must not be negative");
    for (int fn : {desc->m_sim_fn, desc->g_sim_fn})
      if (fn != HRG_SIM_GAUSSIAN && fn != HRG_SIM_TANH) return fail(HRG_ERR_INVALID, "state imitation reward: unknown similarity function");
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  DatasetDev& d = b->ds;
  b->ds_mem.reset();   // the arrays of the dataset before go first: the two never share the device
  d = DatasetDev{};
  b->ds_mem.reset(new DeviceMem());
  DeviceMem& m = *b->ds_mem;
  const size_t n = (size_t)b->n_envs, nep = (size_t)desc->n_episodes, tt = (size_t)desc->total_T;
  std::vector<int32_t> cur(3 * n);   // until the first restore every env follows episode 0 from its first state
  for (size_t e = 0; e < n; e++) { cur[3 * e] = 0; cur[3 * e + 1] = 0; cur[3 * e + 2] = (int32_t)(desc->ep_offset[1] - desc->ep_offset[0]); }
  if (!(m.upload(d.ep_offset, desc->ep_offset, nep + 1) && m.upload(d.states, (const hrg_env_state*)desc->states, tt) &&
        (!desc->boxes || m.upload(d.boxes, (const hrg_box_state*)desc->boxes, tt)) && m.upload(d.obs, desc->obs, HRG_OBS_DIM * (tt + nep)) && m.upload(d.cursor, cur.data(), 3 * n) &&
        m.zeros(d.resets, n) && m.zeros(d.acc, 6 * n) && m.zeros(d.finished, n)))
    return nomem("dataset", m);
  HIPCHK(hipDeviceSynchronize());
  d.n_ep = desc->n_episodes;
  d.total_T = desc->total_T;
  b->dataset = *desc;
  b->dataset.ep_offset = nullptr; b->dataset.states = nullptr; b->dataset.boxes = nullptr; b->dataset.obs = nullptr;
  b->has_dataset = true;
  return HRG_OK;
}

int hrg_batch_dataset_reset(hrg_batch* b, const uint8_t* mask_dev, float* obs_dev, void* stream) {
  if (!b || !obs_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!b->has_dataset) return fail(HRG_ERR_INVALID, "no dataset attached (hrg_batch_dataset_attach)");
  const int rc = hrg_batch_reset(b, mask_dev, obs_dev, stream);
  if (rc != HRG_OK) return rc;
  hipLaunchKernelGGL(hrg_dataset_restore_kernel, dim3((unsigned)b->n_envs), dim3(64), 0, (hipStream_t)stream, b->dataset, b->ds, mask_dev, b->d_states, b->d_boxes, obs_dev,
                     (float*)nullptr, (float*)nullptr, b->env_id0, b->n_envs);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

int hrg_batch_step_dataset(hrg_batch* b, double* actions_dev, float* obs_dev, float* term_obs_dev, float* reward_dev, uint8_t* done_dev, int32_t* info_dev, float* imit_dev,
                           float* sir_dev, void* stream) {
  if (!b || !actions_dev || !obs_dev || !reward_dev || !done_dev || !info_dev || !sir_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!term_obs_dev) return fail(HRG_ERR_INVALID, "hrg_batch_step_dataset needs term_obs_dev: the state a finished env reached is its terminal observation");
  if (!b->has_dataset) return fail(HRG_ERR_INVALID, "no dataset attached (hrg_batch_dataset_attach)");
  const bool air = b->has_expert && b->expert.reward_enabled;
  if (air && !imit_dev) return fail(HRG_ERR_INVALID, "an expert with an imitation reward is attached: imit_dev must not be null");
  const int rc = air ? hrg_batch_step_imitation(b, actions_dev, obs_dev, term_obs_dev, reward_dev, done_dev, info_dev, imit_dev, stream)
                     : hrg_batch_step(b, actions_dev, obs_dev, term_obs_dev, reward_dev, done_dev, info_dev, stream);
  if (rc != HRG_OK) return rc;
  hipLaunchKernelGGL(hrg_sir_post_kernel, dim3((unsigned)((b->n_envs + HRG_DATASET_BLOCK - 1) / HRG_DATASET_BLOCK)), dim3(HRG_DATASET_BLOCK), 0, (hipStream_t)stream, b->dataset, b->ds,
                     (const float*)obs_dev, (const float*)term_obs_dev, reward_dev, done_dev, sir_dev, b->n_envs);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(hrg_dataset_restore_kernel, dim3((unsigned)b->n_envs), dim3(64), 0, (hipStream_t)stream, b->dataset, b->ds, (const uint8_t*)b->ds.finished, b->d_states, b->d_boxes,
                     obs_dev, term_obs_dev, sir_dev, b->env_id0, b->n_envs);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

int hrg_batch_dataset_cursor(hrg_batch* b, int32_t* cursor_host) {
  if (!b || !cursor_host) return fail(HRG_ERR_INVALID, "null argument");
  if (!b->has_dataset) return fail(HRG_ERR_INVALID, "no dataset attached (hrg_batch_dataset_attach)");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(cursor_host, b->ds.cursor, sizeof(int32_t) * 3 * (size_t)b->n_envs, hipMemcpyDeviceToHost));
  return HRG_OK;
}

// ---- test taps: kernels of the base unit on their own ----
int hrg_debug_pose_compare(hrg_batch* b, const void* queries_host, int32_t n, double* out_host) {
  if (!b || !queries_host || !out_host || n <= 0) return fail(HRG_ERR_INVALID, "null argument or n <= 0");
  if (!b->d_pose) return fail(HRG_ERR_UNSUPPORTED, "this batch's task keeps the live tree kinematics (no pose table)");
  DevModel hm;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipMemcpy(&hm, b->d_model, sizeof hm, hipMemcpyDeviceToHost));
  const PoseQuery* qh = (const PoseQuery*)queries_host;
  for (int k = 0; k < n; k++)
    if (qh[k].clip < 0 || qh[k].clip >= hm.clips.n_clips || qh[k].at < 0 || qh[k].at >= hm.clips.clip_len[qh[k].clip]) return fail(HRG_ERR_INVALID, "query outside the clip set");
  const size_t ob = sizeof(double) * 2 * (6 * HRG_NHB + 3 * HRG_NHJ) * (size_t)n;
  const TapBuf in[] = {{qh, sizeof(PoseQuery) * (size_t)n}};
  return tap_result(hrg_run_tap(in, 1, out_host, ob, [&](void** d) {
    hipLaunchKernelGGL(hrg_pose_compare_kernel, dim3((unsigned)n), dim3(64), 0, 0, b->d_model, (const PoseQuery*)d[0], (int)n, (double*)d[1]);
  }), "hrg_debug_pose_compare");
}

int hrg_debug_wave_helpers(const double* in_host, uint64_t lane_mask, double* out_host) {
  if (!in_host || !out_host) return fail(HRG_ERR_INVALID, "null argument");
  const TapBuf in[] = {{in_host, sizeof(double) * 64}};
  return tap_result(hrg_run_tap(in, 1, out_host, sizeof(double) * 64 * HRG_WAVE_NOUT, [&](void** d) {
    hipLaunchKernelGGL(hrg_wave_helpers_kernel, dim3(1), dim3(64), 0, 0, (const double*)d[0], (unsigned long long)lane_mask, (double*)d[1]);
  }), "hrg_debug_wave_helpers");
}

int hrg_debug_cull_box(const double* in_host, int32_t n, double* out_host) {
  if (!in_host || !out_host || n < 1 || n > 16) return fail(HRG_ERR_INVALID, "null argument or n outside 1..16");
  const TapBuf in[] = {{in_host, sizeof(double) * 16 * 7}};
  return tap_result(hrg_run_tap(in, 1, out_host, sizeof(double) * 6, [&](void** d) {
    hipLaunchKernelGGL(hrg_cull_box_kernel, dim3(1), dim3(64), 0, 0, (const double*)d[0], (int)n, (double*)d[1]);
  }), "hrg_debug_cull_box");
}

int hrg_debug_model_constants(hrg_batch* b, double* out_host) {
  if (!b || !out_host) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(b->device));
  return tap_result(hrg_run_tap(nullptr, 0, out_host, sizeof(double) * 2 * HRG_MC_DIM, [&](void** d) {
    hipMemset(d[0], 0, sizeof(double) * 2 * HRG_MC_DIM);
    hipLaunchKernelGGL(hrg_model_constants_tap_kernel, dim3(1), dim3(64), 0, 0, b->d_model, 0.0, (double*)d[0]);
  }), "hrg_debug_model_constants");
}

int hrg_debug_chain_fk(hrg_batch* b, const double* q_host, int32_t n, int32_t shield_on, double* out_host) {
  if (!b || !q_host || !out_host || n < 1 || n > 64) return fail(HRG_ERR_INVALID, "null argument or n outside 1..64");
  HIPCHK(hipSetDevice(b->device));
  void* objs;
  const Variant& v = batch_variant(b, &objs);
  const TapBuf in[] = {{q_host, sizeof(double) * 3 * NARM * (size_t)n}};
  return tap_result(hrg_run_tap(in, 1, out_host, sizeof(double) * HRG_CFK_DIM * (size_t)n, [&](void** d) {
    v.chain_fk((int)n, b->d_model, (const double*)d[0], shield_on ? 1 : 0, (double*)d[1]);
  }), "hrg_debug_chain_fk");
}

int hrg_debug_self_pairs(hrg_batch* b, const double* q_host, int32_t n, double* out_host) {
  if (!b || !q_host || !out_host || n < 1 || n > HRG_SP_MAX) return fail(HRG_ERR_INVALID, "null argument or n outside 1..HRG_SP_MAX");
  HIPCHK(hipSetDevice(b->device));
  void* objs;
  const Variant& v = batch_variant(b, &objs);
  const TapBuf in[] = {{q_host, sizeof(double) * NARM * (size_t)n}};
  return tap_result(hrg_run_tap(in, 1, out_host, sizeof(double) * HRG_SP_DIM * (size_t)n, [&](void** d) {
    v.self_pairs((int)n, b->d_model, (const double*)d[0], (double*)d[1]);
  }), "hrg_debug_self_pairs");
}

int hrg_debug_narrowphase(hrg_batch* b, int32_t kind, const double* queries_host, int32_t n, double* out_host) {
  if (!b || !queries_host || !out_host || n < 1 || n > HRG_NP_MAX) return fail(HRG_ERR_INVALID, "null argument or n outside 1..HRG_NP_MAX");
  if (kind < HRG_NP_SEGSEG || kind > HRG_NP_BOXBOX) return fail(HRG_ERR_INVALID, "no such kind of narrowphase query");
  HIPCHK(hipSetDevice(b->device));
  void* objs;
  const Variant& v = batch_variant(b, &objs);
  bool has = true;
  const TapBuf in[] = {{queries_host, sizeof(double) * HRG_NP_QDIM * (size_t)n}};
  const bool ok = hrg_run_tap(in, 1, out_host, sizeof(double) * HRG_NP_ODIM * (size_t)n, [&](void** d) {
    has = v.narrowphase((int)kind, (int)n, (const double*)d[0], (double*)d[1]) != 0;
  });
  if (!has) return fail(HRG_ERR_UNSUPPORTED, "this batch's kernel variant does not compile that routine");
  return tap_result(ok, "hrg_debug_narrowphase");
}

} // extern "C"
