// hrgym_host_learners.h -- the learners of the C ABI (include/hrgym.h): SAC (hrg_sac_*), PPO (hrg_ppo_*) and the evaluation of their policies (hrg_eval_*), with what
// the two learners check and compute alike; behind them behaviour cloning of their actors (hrg_bc_*) and the DAgger step that fills its table (hrg_dagger_*), and the discriminator of adversarial imitation (hrg_disc_*).  Included by the base unit only, behind hrgym_host.h and hrgym_host_buffers.h (the evaluator reads rows through a buffer's view).

// What both learners check of their networks and batch (csrc/hrgym_mlp.h).  `name`: the learner's message prefix; max_batch: its largest batch.
static int learner_shape(const char* name, int32_t hidden, int32_t depth, int32_t obs_dim, int32_t act_dim, int32_t batch_size, int32_t max_batch) {
  const auto refuse = [name](const char* what, int32_t value, const std::string& why) {
    return fail(HRG_ERR_UNSUPPORTED, std::string(name) + ": " + what + " = " + std::to_string(value) + why);
  };
  if (hidden != HRG_SAC_HIDDEN) return refuse("hidden", hidden, ": the kernels cover hidden width 64 only");
  if (depth < 1 || depth > HRG_SAC_MAX_DEPTH) return refuse("depth", depth, " outside 1 .. 3");
  if (obs_dim < 1 || obs_dim > HRG_OBS_DIM) return refuse("obs_dim", obs_dim, " outside 1 .. HRG_OBS_DIM");
  if (act_dim < 1 || act_dim > HRG_ACT_DIM) return refuse("act_dim", act_dim, " outside 1 .. HRG_ACT_DIM");
  if (batch_size < MLP_T || batch_size > max_batch || batch_size % MLP_T) return refuse("batch_size", batch_size, " is not a multiple of 32 in 32 .. " + std::to_string(max_batch));
  return HRG_OK;
}

// Adam's bias corrections 1 - beta^t for the step after `steps` finished ones (betas 0.9, 0.999)
static void adam_bias_corrections(uint64_t steps, double& bc1, double& bc2) {
  const double t = (double)(steps + 1);
  bc1 = 1.0 - std::pow(0.9, t);
  bc2 = 1.0 - std::pow(0.999, t);
}

// ---- the hyper-parameter table of a population (csrc/hrgym_sac.h: SacHyper, csrc/hrgym_ppo.h: PpoHyper) ----
// rows [n] into table[0 .. n) on `stream`, or rows[0] into every one of them (`same`): launches of hrg_hyper_rows_kernel, a chunk of rows each
template <class Row> static int hyper_upload(Row* table, const Row* rows, int n, bool same, hipStream_t st) {
  for (int first = 0; first < n; first += same ? n : MLP_HYPER_CHUNK) {
    const int count = same ? n : std::min(n - first, (int)MLP_HYPER_CHUNK);
    MlpHyperChunk<Row> c;
    for (int i = 0; i < (same ? 1 : count); i++) c.rows[i] = rows[first + i];
    hipLaunchKernelGGL(hrg_hyper_rows_kernel<Row>, dim3(((unsigned)count + 63) / 64), dim3(64), 0, st, table, first, count, c, same ? 1 : 0);
  }
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

// What a handle keeps of its table on the host: whether the caller set the rows (hrg_*_population_set_hyper: the step's scalar arguments are not read any more), and
// otherwise the row every member holds, written again by the step that is called with other scalars or on another stream than the one the last write was ordered on
// (a handle's steps belong on one stream, as its scratch does; a step that moves to another stream must at least not read a table whose write it is not ordered behind).
template <class Row> struct HyperTable {
  Row* dev = nullptr;       // [n_members]
  bool per_member = false;
  bool filled = false;      // `uniform` is what the table holds, written on `stream`
  Row uniform;
  hipStream_t stream = nullptr;
  int fill(const Row& row, int n, hipStream_t st) {
    if (per_member || (filled && st == stream && std::memcmp(&row, &uniform, sizeof(Row)) == 0)) return HRG_OK;
    if (int rc = hyper_upload(dev, &row, n, true, st)) return rc;
    uniform = row;
    stream = st;
    filled = true;
    return HRG_OK;
  }
  int set(const std::vector<Row>& rows, hipStream_t st) {
    if (int rc = hyper_upload(dev, rows.data(), (int)rows.size(), false, st)) return rc;
    per_member = true;
    return HRG_OK;
  }
};

// "<name>: set_hyper: member <p>: <what>"
static int hyper_refuse(const char* name, int member, const std::string& what) {
  return fail(HRG_ERR_INVALID, std::string(name) + ": set_hyper: member " + std::to_string(member) + ": " + what);
}
static std::string hyper_value(const char* field, double v) { return std::string(field) + " = " + std::to_string(v); }
// the first of the named values that is not finite, or less than its lower bound `lo` (`open`: or equal to it), as "<field> = <value> must be ..."; "" when all pass
struct HyperField { const char* name; double value, lo; bool open; };
static std::string hyper_fields_refusal(std::initializer_list<HyperField> fields) {
  for (const HyperField& f : fields) {
    if (!std::isfinite(f.value)) return hyper_value(f.name, f.value) + " must be finite";
    if (f.value < f.lo || (f.open && f.value == f.lo)) return hyper_value(f.name, f.value) + (f.open ? " must be greater than " : " must not be less than ") + std::to_string(f.lo);
  }
  return "";
}

// what hrg_sac_create checks of the descriptor's values and hrg_sac_population_set_hyper of a row's; "" or what is wrong
static std::string sac_values_refusal(double gamma, double tau, double ent_coef, double target_entropy, int32_t auto_ent_coef) {
  if (!std::isfinite(gamma) || !std::isfinite(tau) || !std::isfinite(ent_coef) || !std::isfinite(target_entropy))
    return "gamma, tau, ent_coef and target_entropy must be finite";
  if (!auto_ent_coef && ent_coef <= 0.0) return "a fixed ent_coef must be positive";
  return "";
}
static SacHyper sac_hyper_row(double learning_rate, double gamma, double tau, double ent_coef, double target_entropy, int32_t auto_ent_coef) {
  SacHyper r;
  r.lr = learning_rate; r.tau = tau;
  r.gamma = (float)gamma; r.alpha_fixed = (float)ent_coef; r.target_entropy = (float)target_entropy;
  r.auto_alpha = auto_ent_coef ? 1 : 0;
  return r;
}

// the same for hrg_ppo_create and hrg_ppo_population_set_hyper
static std::string ppo_values_refusal(double ent_coef, double vf_coef, double max_grad_norm) {
  if (!std::isfinite(ent_coef) || !std::isfinite(vf_coef) || !std::isfinite(max_grad_norm) || ent_coef < 0.0 || vf_coef < 0.0 || max_grad_norm <= 0.0)
    return "ent_coef and vf_coef must be finite and not negative, max_grad_norm finite and positive";
  return "";
}
// ... and of the scheduled values: hrg_ppo_step's arguments, a row's fields
static std::string ppo_schedule_refusal(double learning_rate, double clip_range, double clip_range_vf) {
  if (!std::isfinite(learning_rate) || learning_rate < 0.0) return "learning_rate must be finite and not negative";
  if (!std::isfinite(clip_range) || clip_range <= 0.0) return "clip_range must be finite and positive";
  if (std::isnan(clip_range_vf)) return "clip_range_vf must be a number (negative: no clipping)";
  return "";
}
static PpoHyper ppo_hyper_row(double learning_rate, double clip_range, double clip_range_vf, double ent_coef, double vf_coef, double max_grad_norm) {
  PpoHyper r;
  r.lr = learning_rate; r.clip_range = clip_range; r.clip_range_vf = clip_range_vf < 0.0 ? -1.0 : clip_range_vf;
  r.ent_coef = (float)ent_coef; r.vf_coef = (float)vf_coef; r.max_grad_norm = (float)max_grad_norm;
  return r;
}

extern "C" {

// ---- SAC learner (csrc/hrgym_sac.h) ----
struct hrg_sac {
  int device = 0;
  hrg_sac_desc desc;
  int32_t n_members = 1;    // a population's members (csrc/hrgym_sac.h); the lone learner is the population of one
  SacDev d;
  HyperTable<SacHyper> hyper;   // behind d.hyper
  uint64_t steps = 0;       // gradient steps so far: Adam's step count, the key of the step's draws, the phase of the target update
  uint64_t act_calls = 0;   // act calls that drew their noise
  DeviceMem mem;            // one allocation behind every pointer of `d`
};

// the offsets of the parameter layout (csrc/hrgym_sac.h) into d; returns the number of parameters
static int32_t sac_layout(const hrg_sac_desc& c, SacDev& d) {
  const int32_t K = c.obs_dim, A = c.act_dim, H = HRG_SAC_HIDDEN;
  int32_t o = 0;
  for (int l = 0; l < c.depth; l++) {
    d.a_w[l] = o; o += H * (l ? H : K);
    d.a_b[l] = o; o += H;
  }
  d.a_hw = o; o += 2 * A * H;
  d.a_hb = o; o += 2 * A;
  d.n_actor = o;
  for (int q = 0; q < 2; q++) {
    for (int l = 0; l < c.depth; l++) {
      d.q_w[q][l] = o; o += H * (l ? H : K + A);
      d.q_b[q][l] = o; o += H;
    }
    d.q_ow[q] = o; o += H;
    d.q_ob[q] = o; o += 1;
  }
  d.n_critic = (o - d.n_actor) / 2;
  d.n_params = o + 1;   // log_ent_coef
  return d.n_params;
}

int hrg_sac_population_create(const hrg_sac_desc* desc, int32_t n_members, const uint64_t* seeds, int32_t device, hrg_sac** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_members < 1 || n_members > HRG_SAC_MAX_POPULATION)
    return fail(HRG_ERR_UNSUPPORTED, "sac: n_members = " + std::to_string(n_members) + " outside 1 .. " + std::to_string(HRG_SAC_MAX_POPULATION));
  if (!seeds) return fail(HRG_ERR_INVALID, "sac: a population needs its seeds table (n_members values)");
  if (int rc = learner_shape("sac", desc->hidden, desc->depth, desc->obs_dim, desc->act_dim, desc->batch_size, HRG_SAC_MAX_BATCH)) return rc;
  if (desc->target_update_interval < 1) return fail(HRG_ERR_INVALID, "sac: target_update_interval must be positive");
  const std::string why = sac_values_refusal(desc->gamma, desc->tau, desc->ent_coef, desc->target_entropy, desc->auto_ent_coef);
  if (!why.empty()) return fail(HRG_ERR_INVALID, "sac: " + why);
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_sac> h(new hrg_sac());
  h->device = device;
  h->desc = *desc;
  h->n_members = n_members;
  SacDev& d = h->d;
  d.K = desc->obs_dim; d.A = desc->act_dim; d.depth = desc->depth; d.B = desc->batch_size; d.tiles = desc->batch_size / HRG_SAC_TILE;
  const size_t M = (size_t)n_members, P = (size_t)sac_layout(*desc, d), B = (size_t)d.B, A = (size_t)d.A;   // (the pieces: sac_member)
  Carver<float> f;
  f.take(d.all.a_pi, M * B * A);
  f.take(d.all.logp, M * B);
  f.take(d.all.logp_next, M * B);
  f.take(d.all.y, M * B);
  f.take(d.all.q, M * SAC_NQ * B);
  f.take(d.all.dqda, M * 2 * B * A);
  f.take(d.all.part, M * (size_t)d.tiles * P);
  f.take(d.all.grad, M * P);
  f.take(d.all.loss_part, M * (size_t)d.tiles * SAC_NLOSS);
  f.take(d.all.losses, M * 4);
  if (!f.alloc(h->mem) || !h->mem.upload(d.seeds, seeds, M) || !h->mem.zeros(h->hyper.dev, M)) return nomem("sac", h->mem);
  d.hyper = h->hyper.dev;   // (filled by the first step, or by hrg_sac_population_set_hyper)
  HIPCHK(hipDeviceSynchronize());
  *out = h.release();
  return HRG_OK;
}

int hrg_sac_create(const hrg_sac_desc* desc, int32_t device, hrg_sac** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  return hrg_sac_population_create(desc, 1, &desc->seed, device, out);
}

void hrg_sac_destroy(hrg_sac* h) { destroy_handle(h); }

int hrg_sac_sizes(hrg_sac* h, int64_t* size_host) {
  if (!h || !size_host) return fail(HRG_ERR_INVALID, "null argument");
  size_host[0] = h->d.n_params;
  size_host[1] = h->d.n_actor;
  size_host[2] = h->d.n_critic;
  size_host[3] = (int64_t)h->steps;
  size_host[4] = (int64_t)h->act_calls;
  size_host[5] = (int64_t)h->mem.bytes;
  return HRG_OK;
}

// (a population's step: every array [n_members] times the lone learner's, member p's part at p times its size)
int hrg_sac_step(hrg_sac* h, const float* observations_dev, const float* actions_dev, const float* next_observations_dev, const float* dones_dev, const float* rewards_dev,
                 const float* eps_pi_dev, const float* eps_next_dev, float* params_dev, float* adam_m_dev, float* adam_v_dev, float* target_dev, double learning_rate,
                 void* stream) {
  if (!h || !observations_dev || !actions_dev || !next_observations_dev || !dones_dev || !rewards_dev || !params_dev || !adam_m_dev || !adam_v_dev || !target_dev)
    return fail(HRG_ERR_INVALID, "null argument");
  if (!h->hyper.per_member && (!std::isfinite(learning_rate) || learning_rate < 0.0)) return fail(HRG_ERR_INVALID, "sac: learning_rate must be finite and not negative");
  HIPCHK(hipSetDevice(h->device));
  const SacDev& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  const hrg_sac_desc& c = h->desc;
  if (int rc = h->hyper.fill(sac_hyper_row(learning_rate, c.gamma, c.tau, c.ent_coef, c.target_entropy, c.auto_ent_coef), h->n_members, st)) return rc;
  const unsigned members = (unsigned)h->n_members;
  const dim3 pair((unsigned)d.tiles, 2, members), block(MLP_BLOCK);
  double bc1, bc2;
  adam_bias_corrections(h->steps, bc1, bc2);   // by the optimisers' step count
  const bool polyak = h->steps % (uint64_t)h->desc.target_update_interval == 0;
  const int n_crit2 = 2 * d.n_critic;
  hipLaunchKernelGGL(hrg_sac_policy_kernel, pair, block, 0, st, d, (const float*)params_dev, (const float*)target_dev, observations_dev, next_observations_dev, dones_dev,
                     rewards_dev, eps_pi_dev, eps_next_dev, h->steps);
  hipLaunchKernelGGL(hrg_sac_critic_kernel, pair, block, 0, st, d, (const float*)params_dev, observations_dev, actions_dev);
  hipLaunchKernelGGL(hrg_sac_adam_kernel, dim3(((unsigned)n_crit2 + MLP_BLOCK - 1) / MLP_BLOCK, 1, members), block, 0, st, d, params_dev, adam_m_dev, adam_v_dev, (int)d.n_actor,
                     (int)(d.n_actor + n_crit2), bc1, bc2, polyak ? target_dev : (float*)nullptr, 0);
  hipLaunchKernelGGL(hrg_sac_actor_q_kernel, pair, block, 0, st, d, (const float*)params_dev, observations_dev);
  hipLaunchKernelGGL(hrg_sac_actor_kernel, dim3((unsigned)d.tiles, 1, members), block, 0, st, d, (const float*)params_dev, observations_dev, eps_pi_dev, h->steps);
  hipLaunchKernelGGL(hrg_sac_adam_kernel, dim3(((unsigned)d.n_actor + MLP_BLOCK - 1) / MLP_BLOCK, 1, members), block, 0, st, d, params_dev, adam_m_dev, adam_v_dev, 0, (int)d.n_actor,
                     bc1, bc2, (float*)nullptr, 1);
  HIPCHK(hipGetLastError());
  h->steps++;
  return HRG_OK;
}

int hrg_sac_population_act(hrg_sac* h, const float* params_dev, const float* obs_dev, int32_t n_group, const float* eps_dev, int32_t deterministic, float* actions_dev,
                           void* stream) {
  if (!h || !params_dev || !obs_dev || !actions_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (n_group < 1) return fail(HRG_ERR_INVALID, "sac: n must be positive");
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(hrg_sac_act_kernel, dim3(((unsigned)n_group + MLP_T - 1) / MLP_T, (unsigned)h->n_members), dim3(MLP_BLOCK), 0, (hipStream_t)stream, h->d, params_dev,
                     obs_dev, (int)n_group, eps_dev, (int)(deterministic != 0), h->act_calls, actions_dev);
  HIPCHK(hipGetLastError());
  if (!deterministic && !eps_dev) h->act_calls++;
  return HRG_OK;
}

int hrg_sac_act(hrg_sac* h, const float* params_dev, const float* obs_dev, int32_t n, const float* eps_dev, int32_t deterministic, float* actions_dev, void* stream) {
  if (h && h->n_members != 1) return fail(HRG_ERR_INVALID, "sac: a population of " + std::to_string(h->n_members) + " acts through hrg_sac_population_act (a group of rows per member)");
  return hrg_sac_population_act(h, params_dev, obs_dev, n, eps_dev, deterministic, actions_dev, stream);
}

int hrg_sac_population_export(hrg_sac* h, int32_t member, float* y_host, float* logp_host, float* logp_next_host, float* q_host, float* grad_host, float* losses_host) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  if (member < 0 || member >= h->n_members) return fail(HRG_ERR_INVALID, "sac: member = " + std::to_string(member) + " outside the " + std::to_string(h->n_members) + " members");
  const SacDev& d = h->d;
  const size_t m = (size_t)member, B = (size_t)d.B, P = (size_t)d.n_params;   // (the pieces: sac_member)
  return export_floats(h->device, {{y_host, d.all.y + m * B, B}, {logp_host, d.all.logp + m * B, B}, {logp_next_host, d.all.logp_next + m * B, B},
                                   {q_host, d.all.q + m * SAC_NQ * B, SAC_NQ * B}, {grad_host, d.all.grad + m * P, P}, {losses_host, d.all.losses + m * 4, 4}});
}

int hrg_sac_population_set_hyper(hrg_sac* h, const hrg_sac_hyper* rows_host, int32_t n_members, void* stream) {
  if (!h || !rows_host) return fail(HRG_ERR_INVALID, "sac: set_hyper: null argument");
  if (n_members != h->n_members)
    return fail(HRG_ERR_INVALID, "sac: set_hyper: n_members = " + std::to_string(n_members) + ", the handle has " + std::to_string(h->n_members) + " members");
  std::vector<SacHyper> rows;
  for (int p = 0; p < n_members; p++) {   // every row, before anything is written
    const hrg_sac_hyper& r = rows_host[p];
    const double inf = -std::numeric_limits<double>::infinity();
    std::string why = hyper_fields_refusal({{"learning_rate", r.learning_rate, 0.0, false}, {"gamma", r.gamma, 0.0, false}, {"tau", r.tau, 0.0, false},
                                            {"ent_coef", r.ent_coef, r.auto_ent_coef ? inf : 0.0, !r.auto_ent_coef}, {"target_entropy", r.target_entropy, inf, false}});
    if (why.empty()) why = sac_values_refusal(r.gamma, r.tau, r.ent_coef, r.target_entropy, r.auto_ent_coef);   // (what hrg_sac_create refuses is refused above, by field)
    if (why.empty() && r.gamma > 1.0) why = hyper_value("gamma", r.gamma) + " outside [0, 1]";
    if (why.empty() && r.tau > 1.0) why = hyper_value("tau", r.tau) + " outside [0, 1]";
    if (!why.empty()) return hyper_refuse("sac", p, why);
    rows.push_back(sac_hyper_row(r.learning_rate, r.gamma, r.tau, r.ent_coef, r.target_entropy, r.auto_ent_coef));
  }
  HIPCHK(hipSetDevice(h->device));
  return h->hyper.set(rows, (hipStream_t)stream);
}

int hrg_sac_export(hrg_sac* h, float* y_host, float* logp_host, float* logp_next_host, float* q_host, float* grad_host, float* losses_host) {
  return hrg_sac_population_export(h, 0, y_host, logp_host, logp_next_host, q_host, grad_host, losses_host);
}

// ---- PPO learner (csrc/hrgym_ppo.h) ----
struct hrg_ppo {
  int device = 0;
  hrg_ppo_desc desc;
  int32_t n_members = 1;        // a population's members (csrc/hrgym_ppo.h); the lone learner is the population of one
  PpoDev d;
  HyperTable<PpoHyper> hyper;   // behind d.hyper
  uint64_t steps = 0;           // minibatch steps so far: Adam's step count
  uint64_t forward_calls = 0;   // forward calls that drew their noise
  int n_blocks = 0;             // blocks of 256 parameters
  DeviceMem mem;                // one allocation behind every float pointer of `d`, one behind every double pointer, the seeds table
};

// the offsets of the parameter layout (csrc/hrgym_ppo.h) into d; returns the number of parameters
static int32_t ppo_layout(const hrg_ppo_desc& c, PpoDev& d) {
  const int32_t K = c.obs_dim, A = c.act_dim, H = HRG_PPO_HIDDEN;
  int32_t o = 0;
  for (int n = 0; n < d.nets; n++)
    for (int l = 0; l < c.depth; l++) {
      d.w[n][l] = o; o += H * (l ? H : K);
      d.b[n][l] = o; o += H;
    }
  d.hw = o; o += (A + 1) * H;
  d.hb = o; o += A + 1;
  d.ls = o; o += A;
  d.n_params = o;
  return o;
}

int hrg_ppo_population_create(const hrg_ppo_desc* desc, int32_t n_members, const uint64_t* seeds, int32_t device, hrg_ppo** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_members < 1 || n_members > HRG_PPO_MAX_POPULATION)
    return fail(HRG_ERR_UNSUPPORTED, "ppo: n_members = " + std::to_string(n_members) + " outside 1 .. " + std::to_string(HRG_PPO_MAX_POPULATION));
  if (!seeds) return fail(HRG_ERR_INVALID, "ppo: a population needs its seeds table (n_members values)");
  if (desc->use_sde) return fail(HRG_ERR_UNSUPPORTED, "ppo: use_sde: state dependent exploration is not covered");
  if (desc->target_kl_set) return fail(HRG_ERR_UNSUPPORTED, "ppo: target_kl: the early stop needs a host readback per minibatch");
  if (desc->policy != HRG_PPO_MLP_POLICY) return fail(HRG_ERR_UNSUPPORTED, "ppo: policy = " + std::to_string(desc->policy) + ": the kernels cover MlpPolicy");
  if (int rc = learner_shape("ppo", desc->hidden, desc->depth, desc->obs_dim, desc->act_dim, desc->batch_size, HRG_PPO_MAX_BATCH)) return rc;
  if (desc->separate != 0 && desc->separate != 1) return fail(HRG_ERR_UNSUPPORTED, "ppo: separate must be 0 (shared trunk) or 1 (separate trunks)");
  if (desc->rollout_size < 0 || desc->rollout_size % desc->batch_size)
    return fail(HRG_ERR_UNSUPPORTED, "ppo: rollout_size = " + std::to_string(desc->rollout_size) + " is not divisible by batch_size = " + std::to_string(desc->batch_size) +
                                         ": the learner takes no short last minibatch");
  const std::string why = ppo_values_refusal(desc->ent_coef, desc->vf_coef, desc->max_grad_norm);
  if (!why.empty()) return fail(HRG_ERR_INVALID, "ppo: " + why);
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_ppo> h(new hrg_ppo());
  h->device = device;
  h->desc = *desc;
  h->n_members = n_members;
  PpoDev& d = h->d;
  d.K = desc->obs_dim; d.A = desc->act_dim; d.depth = desc->depth; d.B = desc->batch_size; d.tiles = desc->batch_size / HRG_PPO_TILE;
  d.nets = desc->separate ? 2 : 1;
  d.normalize = desc->normalize_advantage ? 1 : 0;
  const size_t M = (size_t)n_members, P = (size_t)ppo_layout(*desc, d), B = (size_t)d.B;   // (the pieces: ppo_member)
  h->n_blocks = (int)((P + MLP_BLOCK - 1) / MLP_BLOCK);
  Carver<float> f;
  f.take(d.all.values, M * B);
  f.take(d.all.logp, M * B);
  f.take(d.all.ratio, M * B);
  f.take(d.all.part, M * (size_t)d.tiles * P);
  f.take(d.all.grad, M * P);
  f.take(d.all.loss_part, M * (size_t)d.tiles * PPO_NPART);
  f.take(d.all.diag, M * HRG_PPO_NDIAG);
  Carver<double> dbl;
  dbl.take(d.all.adv_stat, M * 2);
  dbl.take(d.all.block_sq, M * (size_t)h->n_blocks);
  if (!f.alloc(h->mem) || !dbl.alloc(h->mem) || !h->mem.upload(d.seeds, seeds, M) || !h->mem.zeros(h->hyper.dev, M)) return nomem("ppo", h->mem);
  d.hyper = h->hyper.dev;   // (filled by the first step, or by hrg_ppo_population_set_hyper)
  HIPCHK(hipDeviceSynchronize());
  *out = h.release();
  return HRG_OK;
}

int hrg_ppo_create(const hrg_ppo_desc* desc, int32_t device, hrg_ppo** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  return hrg_ppo_population_create(desc, 1, &desc->seed, device, out);
}

void hrg_ppo_destroy(hrg_ppo* h) { destroy_handle(h); }

int hrg_ppo_sizes(hrg_ppo* h, int64_t* size_host) {
  if (!h || !size_host) return fail(HRG_ERR_INVALID, "null argument");
  size_host[0] = h->d.n_params;
  size_host[1] = h->d.nets == 2 ? h->d.w[1][0] : h->d.hw;   // (the first network starts at 0)
  size_host[2] = h->d.nets;
  size_host[3] = (int64_t)h->steps;
  size_host[4] = (int64_t)h->forward_calls;
  size_host[5] = (int64_t)h->mem.bytes;
  return HRG_OK;
}

// (a population's step: every array [n_members] times the lone learner's, member p's part at p times its size)
int hrg_ppo_step(hrg_ppo* h, const float* observations_dev, const float* actions_dev, const float* old_values_dev, const float* old_log_prob_dev,
                 const float* advantages_dev, const float* returns_dev, float* params_dev, float* adam_m_dev, float* adam_v_dev, double learning_rate, double clip_range,
                 double clip_range_vf, void* stream) {
  if (!h || !observations_dev || !actions_dev || !old_values_dev || !old_log_prob_dev || !advantages_dev || !returns_dev || !params_dev || !adam_m_dev || !adam_v_dev)
    return fail(HRG_ERR_INVALID, "null argument");
  if (!h->hyper.per_member) {
    const std::string why = ppo_schedule_refusal(learning_rate, clip_range, clip_range_vf);
    if (!why.empty()) return fail(HRG_ERR_INVALID, "ppo: " + why);
  }
  HIPCHK(hipSetDevice(h->device));
  const PpoDev& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  const hrg_ppo_desc& c = h->desc;
  if (int rc = h->hyper.fill(ppo_hyper_row(learning_rate, clip_range, clip_range_vf, c.ent_coef, c.vf_coef, c.max_grad_norm), h->n_members, st)) return rc;
  const unsigned members = (unsigned)h->n_members;
  const dim3 block(MLP_BLOCK), flat((unsigned)h->n_blocks, 1, members);
  double bc1, bc2;
  adam_bias_corrections(h->steps, bc1, bc2);   // by the optimiser's step count
  if (d.normalize) hipLaunchKernelGGL(hrg_ppo_adv_kernel, dim3(1, 1, members), block, 0, st, d, advantages_dev);
  hipLaunchKernelGGL(hrg_ppo_grad_kernel, dim3((unsigned)d.tiles, (unsigned)d.nets, members), block, 0, st, d, (const float*)params_dev, observations_dev, actions_dev, old_values_dev,
                     old_log_prob_dev, advantages_dev, returns_dev);
  hipLaunchKernelGGL(hrg_ppo_reduce_kernel, flat, block, 0, st, d);
  hipLaunchKernelGGL(hrg_ppo_adam_kernel, flat, block, 0, st, d, params_dev, adam_m_dev, adam_v_dev, h->n_blocks, bc1, bc2);
  HIPCHK(hipGetLastError());
  h->steps++;
  return HRG_OK;
}

int hrg_ppo_population_forward(hrg_ppo* h, const float* params_dev, const float* obs_dev, int32_t n_group, const float* eps_dev, int32_t deterministic, float* actions_dev,
                               float* values_dev, float* log_probs_dev, void* stream) {
  if (!h || !params_dev || !obs_dev || !values_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (actions_dev && !log_probs_dev) return fail(HRG_ERR_INVALID, "ppo: actions without log_probs");
  if (n_group < 1) return fail(HRG_ERR_INVALID, "ppo: n must be positive");
  HIPCHK(hipSetDevice(h->device));
  const int value_only = actions_dev ? 0 : 1;
  hipLaunchKernelGGL(hrg_ppo_forward_kernel, dim3(((unsigned)n_group + MLP_T - 1) / MLP_T, value_only ? 1u : (unsigned)h->d.nets, (unsigned)h->n_members), dim3(MLP_BLOCK), 0,
                     (hipStream_t)stream, h->d, params_dev, obs_dev, (int)n_group, eps_dev, (int)(deterministic != 0), h->forward_calls, value_only, actions_dev, values_dev,
                     log_probs_dev);
  HIPCHK(hipGetLastError());
  if (!value_only && !deterministic && !eps_dev) h->forward_calls++;
  return HRG_OK;
}

int hrg_ppo_forward(hrg_ppo* h, const float* params_dev, const float* obs_dev, int32_t n, const float* eps_dev, int32_t deterministic, float* actions_dev,
                    float* values_dev, float* log_probs_dev, void* stream) {
  if (h && h->n_members != 1)
    return fail(HRG_ERR_INVALID, "ppo: a population of " + std::to_string(h->n_members) + " goes forward through hrg_ppo_population_forward (a group of rows per member)");
  return hrg_ppo_population_forward(h, params_dev, obs_dev, n, eps_dev, deterministic, actions_dev, values_dev, log_probs_dev, stream);
}

int hrg_ppo_population_export(hrg_ppo* h, int32_t member, float* values_host, float* log_prob_host, float* ratio_host, float* grad_host, float* diag_host) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  if (member < 0 || member >= h->n_members) return fail(HRG_ERR_INVALID, "ppo: member = " + std::to_string(member) + " outside the " + std::to_string(h->n_members) + " members");
  const PpoDev& d = h->d;
  const size_t m = (size_t)member, B = (size_t)d.B, P = (size_t)d.n_params;   // (the pieces: ppo_member)
  return export_floats(h->device, {{values_host, d.all.values + m * B, B}, {log_prob_host, d.all.logp + m * B, B}, {ratio_host, d.all.ratio + m * B, B},
                                   {grad_host, d.all.grad + m * P, P}, {diag_host, d.all.diag + m * HRG_PPO_NDIAG, HRG_PPO_NDIAG}});
}

int hrg_ppo_population_set_hyper(hrg_ppo* h, const hrg_ppo_hyper* rows_host, int32_t n_members, void* stream) {
  if (!h || !rows_host) return fail(HRG_ERR_INVALID, "ppo: set_hyper: null argument");
  if (n_members != h->n_members)
    return fail(HRG_ERR_INVALID, "ppo: set_hyper: n_members = " + std::to_string(n_members) + ", the handle has " + std::to_string(h->n_members) + " members");
  std::vector<PpoHyper> rows;
  for (int p = 0; p < n_members; p++) {   // every row, before anything is written
    const hrg_ppo_hyper& r = rows_host[p];
    std::string why = hyper_fields_refusal({{"learning_rate", r.learning_rate, 0.0, false}, {"clip_range", r.clip_range, 0.0, true}, {"ent_coef", r.ent_coef, 0.0, false},
                                            {"vf_coef", r.vf_coef, 0.0, false}, {"max_grad_norm", r.max_grad_norm, 0.0, true}});
    if (why.empty() && std::isnan(r.clip_range_vf)) why = hyper_value("clip_range_vf", r.clip_range_vf) + " must be a number (negative: no clipping)";
    if (why.empty()) why = ppo_schedule_refusal(r.learning_rate, r.clip_range, r.clip_range_vf);   // (what hrg_ppo_step and hrg_ppo_create refuse is refused above, by field)
    if (why.empty()) why = ppo_values_refusal(r.ent_coef, r.vf_coef, r.max_grad_norm);
    if (!why.empty()) return hyper_refuse("ppo", p, why);
    rows.push_back(ppo_hyper_row(r.learning_rate, r.clip_range, r.clip_range_vf, r.ent_coef, r.vf_coef, r.max_grad_norm));
  }
  HIPCHK(hipSetDevice(h->device));
  return h->hyper.set(rows, (hipStream_t)stream);
}

int hrg_ppo_export(hrg_ppo* h, float* values_host, float* log_prob_host, float* ratio_host, float* grad_host, float* diag_host) {
  return hrg_ppo_population_export(h, 0, values_host, log_prob_host, ratio_host, grad_host, diag_host);
}

int hrg_sac_restore(hrg_sac* h, uint64_t steps, uint64_t act_calls) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  h->steps = steps;
  h->act_calls = act_calls;
  return HRG_OK;
}

int hrg_ppo_restore(hrg_ppo* h, uint64_t steps, uint64_t forward_calls) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  h->steps = steps;
  h->forward_calls = forward_calls;
  return HRG_OK;
}

// ---- evaluation (csrc/hrgym_eval.h) ----
struct hrg_eval {
  int device = 0;
  hrg_eval_desc desc;
  EvalDev d;
  int64_t steps = 0;   // steps since begin: the finishing step index of the records
  DeviceMem mem;       // behind every pointer of `d`
};

int hrg_eval_create(const hrg_eval_desc* desc, int32_t device, hrg_eval** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  if (desc->n_envs < 1 || desc->n_policies < 1) return fail(HRG_ERR_INVALID, "eval: n_envs and n_policies must be positive");
  if (desc->n_envs % desc->n_policies)
    return fail(HRG_ERR_INVALID, "eval: n_envs = " + std::to_string(desc->n_envs) + " is not divisible by n_policies = " + std::to_string(desc->n_policies) +
                                     ": every parameter set steps a group of the same size");
  if (desc->n_eval_episodes < 1) return fail(HRG_ERR_INVALID, "eval: n_eval_episodes must be positive");
  const int32_t group = desc->n_envs / desc->n_policies;
  const int64_t max_quota = ((int64_t)desc->n_eval_episodes + group - 1) / group;
  if (max_quota > HRG_EVAL_MAX_EPISODES_PER_ENV)
    return fail(HRG_ERR_INVALID, "eval: " + std::to_string(desc->n_eval_episodes) + " episodes over groups of " + std::to_string(group) + " envs are " +
                                     std::to_string(max_quota) + " per env, above HRG_EVAL_MAX_EPISODES_PER_ENV = " + std::to_string(HRG_EVAL_MAX_EPISODES_PER_ENV));
  const int time_col = desc->observe_time ? 1 : 0;
  int width = desc->n_obs_cols + time_col;
  if (desc->goal_env) {
    if (desc->observe_time || desc->normalize) return fail(HRG_ERR_UNSUPPORTED, "eval: goal_env with observe_time or normalize: a goal env's feature row is a plain selection");
    if (desc->goal_kind != HRG_GOAL_REACH && desc->goal_kind != HRG_GOAL_CUBE) return fail(HRG_ERR_UNSUPPORTED, "eval: goal_kind = " + std::to_string(desc->goal_kind));
    width = (desc->goal_kind == HRG_GOAL_REACH ? 6 + 6 : 7 + 3) + desc->n_obs_cols;
    if (width > HRG_OBS_DIM)
      return fail(HRG_ERR_UNSUPPORTED, "eval: a feature row of " + std::to_string(width) + " values; the kernels handle one value per lane, at most HRG_OBS_DIM");
  }
  for (int j = 0; j < HRG_ACT_DIM; j++)
    if (j < desc->act_dim && (!std::isfinite(desc->act_low[j]) || !std::isfinite(desc->act_high[j]) || desc->act_low[j] > desc->act_high[j]))
      return fail(HRG_ERR_INVALID, "eval: act_low and act_high must be finite and ordered");
  double mean[HRG_OBS_DIM], sd[HRG_OBS_DIM];
  if (int rs = view_statistics("eval", desc->n_obs_cols + time_col, desc->normalize, desc->squash, desc->squash_factor, desc->mean, desc->std, mean, sd)) return rs;
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_eval> h(new hrg_eval());
  h->device = device;
  h->desc = *desc;
  EvalDev& d = h->d;
  BufferView& v = d.view;
  DeviceMem& m = h->mem;
  v.observe_time = time_col;
  if (int rc = buffer_columns("eval", desc->n_obs_cols, desc->obs_cols, &desc->observe_time, desc->act_dim, m, v.obs_cols)) return rc;
  v.n_obs_cols = desc->n_obs_cols; v.normalize = desc->normalize ? 1 : 0; v.squash = desc->squash ? 1 : 0; v.squash_factor = desc->squash_factor;
  d.n_envs = desc->n_envs; d.n_policies = desc->n_policies; d.group = group; d.n_episodes = desc->n_eval_episodes; d.max_quota = (int32_t)max_quota;
  d.act_dim = desc->act_dim; d.goal_env = desc->goal_env ? 1 : 0; d.goal_kind = desc->goal_kind; d.width = width;
  const size_t n = (size_t)desc->n_envs;
  if (!(m.zeros(d.ep.cur_obs, n * HRG_OBS_DIM) && m.zeros(d.ep.run_ret, n) && m.zeros(d.ep.run_len, n) && m.zeros(d.cur_time, n) && m.zeros(d.count, n) &&
        m.zeros(d.quota, n) && m.zeros(d.records, n * (size_t)max_quota * HRG_EVAL_RECORD_DIM) && m.zeros(d.remaining, 1) &&
        m.upload(d.act_low, desc->act_low, HRG_ACT_DIM) && m.upload(d.act_high, desc->act_high, HRG_ACT_DIM)))
    return nomem("eval", m);
  if (int ru = view_statistics_upload("eval", m, v, mean, sd)) return ru;
  *out = h.release();
  return HRG_OK;
}

void hrg_eval_destroy(hrg_eval* h) { destroy_handle(h); }

int hrg_eval_begin(hrg_eval* h, const float* obs_dev, const float* time_dev, float* view_dev, void* stream) {
  if (!h || !obs_dev || !view_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (h->d.view.observe_time && !time_dev) return fail(HRG_ERR_INVALID, "eval: observe_time needs the rows' time values");
  HIPCHK(hipSetDevice(h->device));
  h->steps = 0;
  return launch_per_env(hrg_eval_begin_kernel, h->desc.n_envs, stream, h->d, obs_dev, time_dev, view_dev);
}

int hrg_eval_step(hrg_eval* h, const float* obs_dev, const float* reward_dev, const uint8_t* done_dev, const int32_t* info_dev, const float* imit_dev,
                  const float* sir_dev, float* view_dev, void* stream) {
  if (!h || !obs_dev || !reward_dev || !done_dev || !info_dev || !view_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (imit_dev && sir_dev) return fail(HRG_ERR_INVALID, "eval: an imitation row or a state imitation row, not both");
  if (h->d.view.observe_time && !sir_dev) return fail(HRG_ERR_INVALID, "eval: observe_time needs the state imitation rows (their time columns)");
  HIPCHK(hipSetDevice(h->device));
  const int rc = launch_per_env(hrg_eval_step_kernel, h->desc.n_envs, stream, h->d, h->steps, obs_dev, reward_dev, done_dev, info_dev, imit_dev, sir_dev, view_dev);
  if (rc != HRG_OK) return rc;
  h->steps++;
  return HRG_OK;
}

// the actor of a learner by the offsets of its handle, as the evaluator's and the behaviour cloning's kernels take it (csrc/hrgym_eval.h: EvalActor)
static EvalActor sac_actor(const SacDev& s) {
  EvalActor a;
  for (int l = 0; l < HRG_SAC_MAX_DEPTH; l++) { a.w[l] = s.a_w[l]; a.b[l] = s.a_b[l]; }
  a.hw = s.a_hw; a.hb = s.a_hb; a.nout = 2 * s.A;   // (sac_squash reads both heads)
  a.depth = s.depth; a.K = s.K; a.A = s.A; a.n_params = s.n_params;
  return a;
}
static EvalActor ppo_actor(const PpoDev& p) {
  EvalActor a;
  for (int l = 0; l < HRG_PPO_MAX_DEPTH; l++) { a.w[l] = p.w[0][l]; a.b[l] = p.b[0][l]; }   // network 0: the shared trunk, or the policy's
  a.hw = p.hw; a.hb = p.hb; a.nout = p.A;   // the first A rows of the [A + 1][64] heads: action_net
  a.depth = p.depth; a.K = p.K; a.A = p.A; a.n_params = p.n_params;
  return a;
}

// what both policy entries end with: the widths of the learner against the evaluator's, then the launch
static int eval_policy(hrg_eval* h, bool sac, const EvalActor& a, int learner_device, const char* name, const float* params_dev, const float* view_dev, double* actions_dev, void* stream) {
  if (!params_dev || !view_dev || !actions_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (learner_device != h->device)
    return fail(HRG_ERR_INVALID, std::string("eval: the ") + name + " learner lives on device " + std::to_string(learner_device) + ", the evaluator on device " +
                                     std::to_string(h->device));
  if (a.K != h->d.width || a.A != h->d.act_dim)
    return fail(HRG_ERR_INVALID, std::string("eval: the ") + name + " learner takes observations of " + std::to_string(a.K) + " and emits actions of " + std::to_string(a.A) +
                                     " values, the evaluator's view has " + std::to_string(h->d.width) + " and its actions " + std::to_string(h->d.act_dim));
  HIPCHK(hipSetDevice(h->device));
  const dim3 grid(((unsigned)h->d.group + MLP_T - 1) / MLP_T, (unsigned)h->d.n_policies), block(MLP_BLOCK);
  if (sac) hipLaunchKernelGGL(hrg_eval_policy_kernel<true>, grid, block, 0, (hipStream_t)stream, h->d, a, params_dev, view_dev, actions_dev);
  else hipLaunchKernelGGL(hrg_eval_policy_kernel<false>, grid, block, 0, (hipStream_t)stream, h->d, a, params_dev, view_dev, actions_dev);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

int hrg_eval_policy_sac(hrg_eval* h, hrg_sac* sac, const float* params_dev, const float* view_dev, double* actions_dev, void* stream) {
  if (!h || !sac) return fail(HRG_ERR_INVALID, "null argument");
  return eval_policy(h, true, sac_actor(sac->d), sac->device, "sac", params_dev, view_dev, actions_dev, stream);
}

int hrg_eval_policy_ppo(hrg_eval* h, hrg_ppo* ppo, const float* params_dev, const float* view_dev, double* actions_dev, void* stream) {
  if (!h || !ppo) return fail(HRG_ERR_INVALID, "null argument");
  return eval_policy(h, false, ppo_actor(ppo->d), ppo->device, "ppo", params_dev, view_dev, actions_dev, stream);
}

int hrg_eval_remaining(hrg_eval* h, int64_t* remaining_host, void* stream) {
  if (!h || !remaining_host) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(hrg_eval_remaining_kernel, dim3(1), dim3(MLP_BLOCK), 0, st, h->d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(remaining_host, h->d.remaining, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return HRG_OK;
}

int hrg_eval_export(hrg_eval* h, int32_t* counts_host, int32_t* quota_host, double* records_host) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  const EvalDev& d = h->d;
  const size_t n = (size_t)d.n_envs;
  if (counts_host) HIPCHK(hipMemcpy(counts_host, d.count, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (quota_host) HIPCHK(hipMemcpy(quota_host, d.quota, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (records_host) HIPCHK(hipMemcpy(records_host, d.records, n * (size_t)d.max_quota * HRG_EVAL_RECORD_DIM * sizeof(double), hipMemcpyDeviceToHost));
  return HRG_OK;
}

int hrg_eval_size(hrg_eval* h, int64_t* size_host) {
  if (!h || !size_host) return fail(HRG_ERR_INVALID, "null argument");
  size_host[0] = h->d.max_quota;
  size_host[1] = h->steps;
  size_host[2] = h->d.width;
  size_host[3] = (int64_t)h->mem.bytes;
  return HRG_OK;
}

// ---- behaviour cloning (csrc/hrgym_bc.h) ----
struct hrg_bc {
  int device = 0;
  hrg_bc_desc desc;
  BcDev d;
  uint64_t steps = 0;   // bc steps so far: Adam's step count and the key of the step's draws
  DeviceMem mem;        // behind every pointer of `d`
};

// what both create entries end with: `a` the learner's actor (sac_actor / ppo_actor), the learner's device and members
static int bc_create(const hrg_bc_desc* desc, int32_t kind, EvalActor a, int learner_device, int32_t n_members, int32_t device, hrg_bc** out) {
  if (desc->kind != kind)
    return fail(HRG_ERR_INVALID, "bc: kind = " + std::to_string(desc->kind) + ": this entry creates from " + (kind == HRG_BC_SAC ? "an hrg_sac (HRG_BC_SAC)" : "an hrg_ppo (HRG_BC_PPO)"));
  if (n_members != 1) return fail(HRG_ERR_UNSUPPORTED, "bc: a population of " + std::to_string(n_members) + " members: behaviour cloning covers lone learners");
  if (device != learner_device)
    return fail(HRG_ERR_INVALID, "bc: the learner lives on device " + std::to_string(learner_device) + ", not on device " + std::to_string(device));
  if (int rc = learner_shape("bc", HRG_SAC_HIDDEN, a.depth, a.K, a.A, desc->batch_size, HRG_BC_MAX_BATCH)) return rc;
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_bc> h(new hrg_bc());
  h->device = device;
  h->desc = *desc;
  BcDev& d = h->d;
  a.nout = a.A;   // the mean head alone: the first A rows of the learner's head product
  d.a = a;
  d.sac = kind == HRG_BC_SAC ? 1 : 0;
  d.B = desc->batch_size; d.tiles = desc->batch_size / HRG_SAC_TILE; d.seed = desc->seed;
  d.lo[0] = a.w[0]; d.n[0] = a.b[a.depth - 1] + MLP_H - a.w[0];   // a network's layers lie one behind the other: W_0, b_0, W_1, ..
  d.lo[1] = a.hw; d.n[1] = a.A * MLP_H;
  d.lo[2] = a.hb; d.n[2] = a.A;
  d.n_reach = d.n[0] + d.n[1] + d.n[2];
  const size_t P = (size_t)a.n_params, B = (size_t)d.B;
  Carver<float> f;
  f.take(d.pred, B * (size_t)a.A);
  f.take(d.part, (size_t)d.tiles * P);
  f.take(d.grad, P);
  f.take(d.loss_part, (size_t)d.tiles);
  f.take(d.loss, 1);
  if (!f.alloc(h->mem) || !h->mem.zeros(d.index, B)) return nomem("bc", h->mem);
  HIPCHK(hipDeviceSynchronize());
  *out = h.release();
  return HRG_OK;
}

int hrg_bc_create_sac(const hrg_bc_desc* desc, hrg_sac* learner, int32_t device, hrg_bc** out) {
  if (!desc || !learner || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  return bc_create(desc, HRG_BC_SAC, sac_actor(learner->d), learner->device, learner->n_members, device, out);
}

int hrg_bc_create_ppo(const hrg_bc_desc* desc, hrg_ppo* learner, int32_t device, hrg_bc** out) {
  if (!desc || !learner || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  return bc_create(desc, HRG_BC_PPO, ppo_actor(learner->d), learner->device, learner->n_members, device, out);
}

void hrg_bc_destroy(hrg_bc* h) { destroy_handle(h); }

int hrg_bc_sizes(hrg_bc* h, int64_t* size_host) {
  if (!h || !size_host) return fail(HRG_ERR_INVALID, "null argument");
  size_host[0] = h->d.n_reach;
  size_host[1] = (int64_t)h->steps;
  size_host[2] = h->d.a.n_params;
  size_host[3] = (int64_t)h->mem.bytes;
  return HRG_OK;
}

int hrg_bc_step(hrg_bc* h, const float* table_obs_dev, const float* table_act_dev, int64_t n_rows, const int64_t* index_in_dev, float* params_dev, float* bc_m_dev,
                float* bc_v_dev, double learning_rate, void* stream) {
  if (!h || !params_dev || !bc_m_dev || !bc_v_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!table_obs_dev || !table_act_dev) return fail(HRG_ERR_INVALID, "bc: null table (observations and actions of n_rows rows)");
  if (n_rows < 1) return fail(HRG_ERR_INVALID, "bc: n_rows = " + std::to_string(n_rows) + " must be positive");
  if (!std::isfinite(learning_rate) || learning_rate < 0.0) return fail(HRG_ERR_INVALID, "bc: learning_rate must be finite and not negative");
  HIPCHK(hipSetDevice(h->device));
  const BcDev& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  double bc1, bc2;
  adam_bias_corrections(h->steps, bc1, bc2);
  hipLaunchKernelGGL(hrg_bc_grad_kernel, dim3((unsigned)d.tiles), dim3(MLP_BLOCK), 0, st, d, (const float*)params_dev, table_obs_dev, table_act_dev, n_rows, index_in_dev, h->steps);
  hipLaunchKernelGGL(hrg_bc_adam_kernel, dim3(((unsigned)d.n_reach + MLP_BLOCK - 1) / MLP_BLOCK), dim3(MLP_BLOCK), 0, st, d, params_dev, bc_m_dev, bc_v_dev, learning_rate, bc1, bc2);
  HIPCHK(hipGetLastError());
  h->steps++;
  return HRG_OK;
}

int hrg_bc_export(hrg_bc* h, int64_t* index_host, float* pred_host, float* grad_host, float* loss_host) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  const BcDev& d = h->d;
  if (int rc = export_floats(h->device, {{pred_host, d.pred, (size_t)d.B * (size_t)d.a.A}, {grad_host, d.grad, (size_t)d.a.n_params}, {loss_host, d.loss, 1}})) return rc;
  if (index_host) HIPCHK(hipMemcpy(index_host, d.index, (size_t)d.B * sizeof(int64_t), hipMemcpyDeviceToHost));
  return HRG_OK;
}

// ---- DAgger (csrc/hrgym_dagger.h) ----
struct hrg_dagger {
  int device = 0;
  hrg_dagger_desc desc;
  DaggerDev d;
  uint64_t calls = 0;   // steps so far: the key of the next step's draws
  int32_t slot = 0;     // the next step slot (the write position lives on the host)
  DeviceMem mem;        // behind every pointer of `d`
};

int hrg_dagger_create(const hrg_dagger_desc* desc, int32_t device, hrg_dagger** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  if (desc->kind != HRG_BC_SAC && desc->kind != HRG_BC_PPO) return fail(HRG_ERR_INVALID, "dagger: kind = " + std::to_string(desc->kind) + ": HRG_BC_SAC or HRG_BC_PPO");
  if (desc->n_envs < 1) return fail(HRG_ERR_INVALID, "dagger: n_envs = " + std::to_string(desc->n_envs) + " must be positive");
  if (desc->obs_dim < 1 || desc->obs_dim > HRG_OBS_DIM) return fail(HRG_ERR_UNSUPPORTED, "dagger: obs_dim = " + std::to_string(desc->obs_dim) + " outside 1 .. HRG_OBS_DIM");
  if (desc->act_dim < 1 || desc->act_dim > HRG_ACT_DIM) return fail(HRG_ERR_UNSUPPORTED, "dagger: act_dim = " + std::to_string(desc->act_dim) + " outside 1 .. HRG_ACT_DIM");
  if (desc->capacity_steps < 1) return fail(HRG_ERR_INVALID, "dagger: capacity_steps = " + std::to_string(desc->capacity_steps) + " must be positive");
  if (desc->pinned_rows < 0) return fail(HRG_ERR_INVALID, "dagger: pinned_rows = " + std::to_string(desc->pinned_rows) + " must not be negative");
  for (int j = 0; j < desc->act_dim; j++)
    if (!std::isfinite(desc->act_low[j]) || !std::isfinite(desc->act_high[j]) || desc->act_high[j] <= desc->act_low[j])
      return fail(HRG_ERR_INVALID, "dagger: action bound " + std::to_string(j) + ": act_low and act_high must be finite with act_high > act_low");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_dagger> h(new hrg_dagger());
  h->device = device;
  h->desc = *desc;
  DaggerDev& d = h->d;
  d.sac = desc->kind == HRG_BC_SAC ? 1 : 0;
  d.n = desc->n_envs; d.K = desc->obs_dim; d.A = desc->act_dim; d.pinned = desc->pinned_rows;
  d.env_id0 = desc->env_id0; d.seed = desc->seed;
  if (!h->mem.upload(d.low, desc->act_low, HRG_ACT_DIM) || !h->mem.upload(d.high, desc->act_high, HRG_ACT_DIM) ||
      !h->mem.zeros(d.stats, (size_t)d.n * HRG_DAGGER_STATS_DIM))
    return nomem("dagger", h->mem);
  HIPCHK(hipDeviceSynchronize());
  *out = h.release();
  return HRG_OK;
}

void hrg_dagger_destroy(hrg_dagger* h) { destroy_handle(h); }

int hrg_dagger_sizes(hrg_dagger* h, int64_t* size_host) {
  if (!h || !size_host) return fail(HRG_ERR_INVALID, "null argument");
  size_host[0] = (int64_t)h->calls;
  size_host[1] = h->slot;
  size_host[2] = (int64_t)h->desc.pinned_rows + (int64_t)std::min<uint64_t>(h->calls, (uint64_t)h->desc.capacity_steps) * (int64_t)h->desc.n_envs;
  size_host[3] = (int64_t)h->mem.bytes;
  return HRG_OK;
}

int hrg_dagger_step(hrg_dagger* h, const float* view_dev, const float* learner_act_dev, const double* expert_act_dev, double beta, float* table_obs_dev,
                    float* table_act_dev, double* rows_out_dev, float* kept_out_dev, void* stream) {
  if (!h || !view_dev || !learner_act_dev || !expert_act_dev || !rows_out_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!table_obs_dev || !table_act_dev) return fail(HRG_ERR_INVALID, "dagger: null table (observations and actions of pinned_rows + capacity_steps * n_envs rows)");
  if (!(beta >= 0.0 && beta <= 1.0)) return fail(HRG_ERR_INVALID, "dagger: beta = " + std::to_string(beta) + " outside [0, 1]");
  HIPCHK(hipSetDevice(h->device));
  const int rc = launch_per_wave(hrg_dagger_step_kernel, h->desc.n_envs, stream, h->d, view_dev, learner_act_dev, expert_act_dev, beta, h->calls, (int64_t)h->slot, table_obs_dev,
                                 table_act_dev, rows_out_dev, kept_out_dev);
  if (rc) return rc;
  h->calls++;
  if (++h->slot == h->desc.capacity_steps) h->slot = 0;   // the oldest step is overwritten
  return HRG_OK;
}

int hrg_dagger_stats(hrg_dagger* h, double* per_env_host, int32_t clear) {
  if (!h || !per_env_host) return fail(HRG_ERR_INVALID, "null argument");
  return buffer_stats(h->device, h->d.stats, h->desc.n_envs, HRG_DAGGER_STATS_DIM, per_env_host, clear);
}

// ---- adversarial imitation: the discriminator (csrc/hrgym_disc.h) ----
struct hrg_disc {
  int device = 0;
  hrg_disc_desc desc;
  DiscDev d;
  uint64_t steps = 0;   // updates so far: Adam's step count and the key of the step's draws
  DeviceMem mem;        // behind every pointer of `d`
};

int hrg_disc_create(const hrg_disc_desc* desc, int32_t device, hrg_disc** out) {
  if (!desc || !out) return fail(HRG_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = learner_shape("disc", desc->hidden, desc->depth, desc->obs_dim, desc->act_dim, desc->batch_size, HRG_DISC_MAX_BATCH)) return rc;
  if (desc->activation != HRG_DISC_RELU && desc->activation != HRG_DISC_TANH)
    return fail(HRG_ERR_INVALID, "disc: activation = " + std::to_string(desc->activation) + ": HRG_DISC_RELU or HRG_DISC_TANH");
  if (desc->reward_kind != HRG_DISC_REWARD_GAIL && desc->reward_kind != HRG_DISC_REWARD_AIRL)
    return fail(HRG_ERR_INVALID, "disc: reward_kind = " + std::to_string(desc->reward_kind) + ": HRG_DISC_REWARD_GAIL or HRG_DISC_REWARD_AIRL");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<hrg_disc> h(new hrg_disc());
  h->device = device;
  h->desc = *desc;
  DiscDev& d = h->d;
  d.K = desc->obs_dim; d.A = desc->act_dim; d.depth = desc->depth; d.B = desc->batch_size; d.tiles = 2 * desc->batch_size / HRG_SAC_TILE;
  d.unit = desc->activation == HRG_DISC_RELU ? MLP_ACT_RELU : MLP_ACT_TANH; d.kind = desc->reward_kind; d.seed = desc->seed;
  int32_t o = 0;
  for (int l = 0; l < d.depth; l++) {
    d.w[l] = o; o += MLP_H * (l ? MLP_H : d.K + d.A);
    d.b[l] = o; o += MLP_H;
  }
  d.hw = o; o += MLP_H;
  d.hb = o; o += 1;
  d.n_params = o;
  const size_t P = (size_t)d.n_params, B = (size_t)d.B;
  Carver<float> f;
  f.take(d.logits, 2 * B);
  f.take(d.part, (size_t)d.tiles * P);
  f.take(d.grad, P);
  f.take(d.stat_part, (size_t)d.tiles * DISC_NSTAT);
  f.take(d.diag, 3);
  if (!f.alloc(h->mem) || !h->mem.zeros(d.index, B)) return nomem("disc", h->mem);
  HIPCHK(hipDeviceSynchronize());
  *out = h.release();
  return HRG_OK;
}

void hrg_disc_destroy(hrg_disc* h) { destroy_handle(h); }

int hrg_disc_sizes(hrg_disc* h, int64_t* size_host) {
  if (!h || !size_host) return fail(HRG_ERR_INVALID, "null argument");
  size_host[0] = h->d.n_params;
  size_host[1] = (int64_t)h->steps;
  size_host[2] = h->d.tiles;
  size_host[3] = h->d.B;
  return HRG_OK;
}

int hrg_disc_step(hrg_disc* h, const float* table_obs_dev, const float* table_act_dev, int64_t n_rows, const int64_t* index_in_dev, const float* policy_obs_dev,
                  const float* policy_act_dev, float* params_dev, float* m_dev, float* v_dev, double learning_rate, void* stream) {
  if (!h || !policy_obs_dev || !policy_act_dev || !params_dev || !m_dev || !v_dev) return fail(HRG_ERR_INVALID, "null argument");
  if (!table_obs_dev || !table_act_dev) return fail(HRG_ERR_INVALID, "disc: null table (observations and actions of n_rows rows)");
  if (n_rows < 1) return fail(HRG_ERR_INVALID, "disc: n_rows = " + std::to_string(n_rows) + " must be positive");
  if (!std::isfinite(learning_rate) || learning_rate < 0.0) return fail(HRG_ERR_INVALID, "disc: learning_rate must be finite and not negative");
  HIPCHK(hipSetDevice(h->device));
  const DiscDev& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  double bc1, bc2;
  adam_bias_corrections(h->steps, bc1, bc2);
  hipLaunchKernelGGL(hrg_disc_grad_kernel, dim3((unsigned)d.tiles), dim3(MLP_BLOCK), 0, st, d, (const float*)params_dev, table_obs_dev, table_act_dev, n_rows, index_in_dev,
                     policy_obs_dev, policy_act_dev, h->steps);
  hipLaunchKernelGGL(hrg_disc_adam_kernel, dim3(((unsigned)d.n_params + MLP_BLOCK - 1) / MLP_BLOCK), dim3(MLP_BLOCK), 0, st, d, params_dev, m_dev, v_dev, learning_rate, bc1, bc2);
  HIPCHK(hipGetLastError());
  h->steps++;
  return HRG_OK;
}

int hrg_disc_reward(hrg_disc* h, const float* params_dev, const float* obs_dev, const float* act_dev, int32_t n, const float* env_rewards_dev, double alpha,
                    float* rewards_out_dev, float* logits_out_dev, void* stream) {
  if (!h || !params_dev || !obs_dev || !act_dev || (!rewards_out_dev && !logits_out_dev)) return fail(HRG_ERR_INVALID, "null argument");
  if (n < 1) return fail(HRG_ERR_INVALID, "disc: n = " + std::to_string(n) + " must be positive");
  if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(HRG_ERR_INVALID, "disc: alpha = " + std::to_string(alpha) + " outside [0, 1]");
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(hrg_disc_reward_kernel, dim3(((unsigned)n + MLP_T - 1) / MLP_T), dim3(MLP_BLOCK), 0, (hipStream_t)stream, h->d, params_dev, obs_dev, act_dev, (int)n,
                     env_rewards_dev, alpha, rewards_out_dev, logits_out_dev);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}

int hrg_disc_export(hrg_disc* h, int64_t* index_host, float* logits_host, float* grad_host, float* diag_host) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  const DiscDev& d = h->d;
  if (int rc = export_floats(h->device, {{logits_host, d.logits, 2 * (size_t)d.B}, {grad_host, d.grad, (size_t)d.n_params}, {diag_host, d.diag, 3}})) return rc;
  if (index_host) HIPCHK(hipMemcpy(index_host, d.index, (size_t)d.B * sizeof(int64_t), hipMemcpyDeviceToHost));
  return HRG_OK;
}

int hrg_disc_restore(hrg_disc* h, uint64_t steps) {
  if (!h) return fail(HRG_ERR_INVALID, "null argument");
  h->steps = steps;
  return HRG_OK;
}

} // extern "C"
