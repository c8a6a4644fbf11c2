// carl_ppo_sets.hip -- C-ABI entry points of a POPULATION of PPO learners (include/carl_amd.h: carl_ppo_grad_sets,
// carl_ppo_adv_stats_sets, carl_adam_step_sets) and their launches.  A translation unit of its own, so that every other
// unit's kernels compile exactly as they did.  The kernels are ppo_sets_kernels.hip.h's: the one-set kernels' bodies, run
// once per member.  The checks and their messages are ppo_host_checks.hpp's and ppo_step_host.hpp's, which the one-set entry
// points share; what is added here is what only a population can get wrong.
#include "classic_control.hip.h"
#include "policy_launch.hpp"
#include "ppo_host_checks.hpp"
#include "ppo_sets_kernels.hip.h"
#include "ppo_step_host.hpp"

namespace {

using carl_host::check_launch;
using carl_host::fail;

constexpr int kMaxSets = 65535;  // the second grid dimension (the Adam launch, one workgroup per member, keeps to it too)

// the member count of any of the three calls
int check_n_sets(const char* who, int n_sets) {
  if (n_sets < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_sets %d < 1", who, n_sets);
  if (n_sets > kMaxSets)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_sets %d > %d (the second grid dimension)", who, n_sets, kMaxSets);
  return 0;
}

// a network's weight sets against the buffer: n_sets members of lanes_per_set lanes that tile the lanes exactly
int check_sets(const char* who, const carl_policy_t* p, const carl_ppo_batch_t* ppo) {
  if (int e = check_n_sets(who, p->n_sets)) return e;
  const int q = carl_policy_lane_quantum();
  if (p->lanes_per_set < q || p->lanes_per_set % q != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: lanes_per_set %d is not a positive multiple of %d (carl_policy_lane_quantum)",
                who, p->lanes_per_set, q);
  if ((int64_t)p->n_sets * p->lanes_per_set != ppo->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d sets x %d lanes are not the buffer's %d lanes (member s owns lanes "
                "[s * lanes_per_set, (s + 1) * lanes_per_set))", who, p->n_sets, p->lanes_per_set, ppo->n_lanes);
  return carl_host::check_params(who, p);
}

// one-set slab floats of both networks for n_samples samples
int64_t member_workspace_floats(const carl_policy_t* policy, const carl_policy_t* critic, int32_t n_samples) {
  return (int64_t)carl_host::ppo_workgroups(n_samples) *
         (carl::ppo_slab_floats(carl_host::policy_padded_hidden(policy)) +
          carl::ppo_slab_floats(carl_host::policy_padded_hidden(critic)));
}

// ppo_net_sets_kernel<H> for a network of padded hidden width H over (grid, n_sets) workgroups
int launch_net_sets(const char* who, int H, const carl::PpoNetArgs& a, const carl::PpoSetsArgs& p, int grid, int n_sets,
                    hipStream_t s) {
  return carl_host::with_padded_hidden(H, [&](auto h) {
    constexpr int kH = decltype(h)::value;
    void (*fn)(carl::PpoNetArgs, carl::PpoSetsArgs) = carl::ppo_net_sets_kernel<kH>;
    if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(fn), carl::ppo_lds_bytes(kH), who)) return e;
    hipLaunchKernelGGL(fn, dim3(grid, n_sets), dim3(carl::kPpoThreads), carl::ppo_lds_bytes(kH), s, a, p);
    return check_launch(who);
  });
}

}  // namespace

extern "C" {

int64_t carl_ppo_sets_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples) {
  if (policy_host == nullptr || critic_host == nullptr || n_samples < 1 || policy_host->n_sets < 1) return -1;
  if (carl_host::policy_set_floats(policy_host) < 0 || carl_host::policy_set_floats(critic_host) < 0) return -1;
  return (int64_t)policy_host->n_sets * member_workspace_floats(policy_host, critic_host, n_samples);
}

int carl_ppo_grad_sets(const carl_ppo_batch_t* ppo, const carl_policy_t* policy_host, const carl_policy_t* critic_host,
                       const float* log_std, const carl_ppo_sets_t* sets, const carl_ppo_out_t* out, void* stream) {
  const char* who = "carl_ppo_grad_sets";
  if (ppo == nullptr || policy_host == nullptr || critic_host == nullptr || sets == nullptr || out == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ppo / policy / critic / sets / out is NULL", who);
  carl_family_info_t fi;
  if (int e = carl_host::check_ppo_classic_buffer(who, ppo, &fi)) return e;
  const int want_out = fi.action_is_discrete ? fi.n_actions : 1;
  if (int e = carl_host::check_ppo_classic_network(who, policy_host, fi, want_out,
                                                   fi.action_is_discrete ? "n_actions" : "one Box value")) return e;
  if (policy_host->head != (fi.action_is_discrete ? CARL_POLICY_HEAD_ARGMAX : CARL_POLICY_HEAD_BOX))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head kind %d does not match the family's action space", who,
                policy_host->head);
  if (int e = check_sets(who, policy_host, ppo)) return e;
  const char* cwho = "carl_ppo_grad_sets: critic";
  if (int e = carl_host::check_ppo_classic_network(cwho, critic_host, fi, 1, "a value network has 1")) return e;
  if (int e = carl_host::check_ppo_critic_inputs(cwho, critic_host, policy_host)) return e;
  if (critic_host->n_sets != policy_host->n_sets || critic_host->lanes_per_set != policy_host->lanes_per_set)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d sets x %d lanes, the actor has %d x %d", cwho, critic_host->n_sets,
                critic_host->lanes_per_set, policy_host->n_sets, policy_host->lanes_per_set);
  if (int e = carl_host::check_params(cwho, critic_host)) return e;
  if (int e = carl_host::check_ppo_classic_action(who, ppo, fi)) return e;
  const int P = policy_host->n_sets, L = policy_host->lanes_per_set;
  if (sets->hyper == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sets->hyper is NULL", who);
  if (sets->idx == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sets->idx is NULL (every member's minibatch is a row of indices)", who);
  if (sets->idx_set_stride < ppo->n_samples)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: idx_set_stride %lld < n_samples %d", who, (long long)sets->idx_set_stride,
                ppo->n_samples);
  if (sets->adv_norm != nullptr && sets->adv_norm_set_stride < 2)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: adv_norm_set_stride %lld < 2", who, (long long)sets->adv_norm_set_stride);
  // the buffer and the outputs as carl_ppo_grad checks them; its coefficients, idx and adv_norm are not read here
  carl_ppo_batch_t b = *ppo;
  b.clip_range = b.vf_coef = b.ent_coef = 0.0f;
  b.idx = sets->idx, b.adv_norm = nullptr;
  const int pitch = ppo->row_pitch > 0 ? ppo->row_pitch : ppo->n_lanes;
  if (int e = carl_host::check_ppo_batch(who, &b, pitch, out)) return e;
  if (ppo->n_samples > (int64_t)ppo->n_steps * L)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_samples %d > n_steps %d x lanes_per_set %d (a member's minibatch is drawn "
                "from its own lanes)", who, ppo->n_samples, ppo->n_steps, L);
  if (!fi.action_is_discrete && (log_std == nullptr || out->grad_log_std == nullptr))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a Box family needs log_std and out->grad_log_std ([n_sets] on the device)", who);
  if (out->new_log_prob != nullptr || out->new_value != nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out->new_log_prob / out->new_value are not offered for a population (NULL)", who);
  const int64_t need = carl_ppo_sets_workspace_floats(policy_host, critic_host, ppo->n_samples);
  if (int e = carl_host::check_ppo_workspace(who, out, need, "carl_ppo_sets_workspace_floats")) return e;

  const hipStream_t s = (hipStream_t)stream;
  const int grid = carl_host::ppo_workgroups(ppo->n_samples);
  const int ha = carl_host::policy_padded_hidden(policy_host), hc = carl_host::policy_padded_hidden(critic_host);
  const int64_t slab_a = (int64_t)grid * carl::ppo_slab_floats(ha), slab_c = (int64_t)grid * carl::ppo_slab_floats(hc);
  const int actor_kind = fi.action_is_discrete ? carl::kPpoCategorical : carl::kPpoGaussian;
  // member s's slabs: the actor's [P][grid], then the critic's [P][grid]
  carl::PpoNetArgs a{};
  a.b = b;
  a.b.idx = nullptr;  // (the kernels read the member's row of sets->idx)
  a.b.row_pitch = pitch;
  a.n_ctx = policy_host->n_ctx;
  for (int k = 0; k < policy_host->n_ctx; ++k) a.ctx_rows[k] = policy_host->ctx_rows[k];
  a.xform = policy_host->params + carl_host::policy_transform_offset(policy_host);
  a.log_std = log_std;
  a.n_tiles = (ppo->n_samples + carl::kPpoTile - 1) / carl::kPpoTile;
  a.shape = carl_host::ppo_shape_of(policy_host, carl_host::policy_set_floats);
  a.kind = actor_kind;
  a.params = policy_host->params;
  a.slab = out->workspace;
  a.new_out = nullptr;
  carl::PpoSetsArgs ps{};
  ps.hyper = sets->hyper, ps.idx = sets->idx, ps.adv_norm = sets->adv_norm;
  ps.idx_stride = sets->idx_set_stride, ps.adv_stride = sets->adv_norm_set_stride;
  ps.slab_stride = slab_a;
  ps.lanes_per_set = L;
  ps.xform_stride = a.shape.set_floats;
  if (int e = launch_net_sets(who, ha, a, ps, grid, P, s)) return e;
  // the critic, on the actor's transformed inputs
  carl::PpoNetArgs c = a;
  c.shape = carl_host::ppo_shape_of(critic_host, carl_host::policy_set_floats);
  c.kind = carl::kPpoValue;
  c.params = critic_host->params;
  c.slab = out->workspace + (size_t)P * slab_a;
  carl::PpoSetsArgs pc = ps;
  pc.slab_stride = slab_c;
  if (int e = launch_net_sets(who, hc, c, pc, grid, P, s)) return e;
  // every member's slabs, in workgroup order
  carl::PpoReduceArgs r{};
  r.actor = a.shape, r.critic = c.shape;
  r.h_actor = ha, r.h_critic = hc;
  r.n_workgroups = grid;
  r.gaussian = actor_kind == carl::kPpoGaussian ? 1 : 0;
  r.inv_m = 1.0 / (double)ppo->n_samples;
  r.n_samples = (float)ppo->n_samples;
  r.slab_actor = a.slab, r.slab_critic = c.slab;
  r.grad_actor = out->grad_actor, r.grad_critic = out->grad_critic, r.grad_log_std = out->grad_log_std;
  r.stats = out->stats;
  const carl::PpoReduceSetsArgs rs{slab_a, slab_c};
  const int outputs = r.actor.set_floats + r.critic.set_floats + 8;
  hipLaunchKernelGGL(carl::ppo_reduce_sets_kernel, dim3((outputs + 255) / 256, P), dim3(256), 0, s, r, rs);
  return check_launch(who);
}

int carl_ppo_adv_stats_sets(const carl_ppo_adv_stats_t* as, int32_t n_sets, int64_t idx_set_stride, void* stream) {
  const char* who = "carl_ppo_adv_stats_sets";
  if (int e = carl_host::check_adv_stats(who, as)) return e;
  if (int e = check_n_sets(who, n_sets)) return e;
  if (idx_set_stride < as->n_total)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: idx_set_stride %lld < n_total %d", who, (long long)idx_set_stride, as->n_total);
  const carl::PpoAdvStatsArgs a = carl_host::adv_stats_args(as);
  hipLaunchKernelGGL(carl::ppo_adv_stats_sets_kernel, dim3(carl_host::adv_rows(as->n_total, as->batch_size), n_sets),
                     dim3(carl::kAdvThreads), 0, (hipStream_t)stream, a, (long long)idx_set_stride);
  return check_launch(who);
}

int carl_adam_step_sets(const carl_adam_t* ad, int32_t n_sets, const double* hyper, void* stream) {
  const char* who = "carl_adam_step_sets";
  int64_t total = 0;
  if (int e = carl_host::check_adam(who, ad, false, &total)) return e;
  if (int e = check_n_sets(who, n_sets)) return e;
  if (hyper == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: hyper is NULL (lr and max_grad_norm are read from the device)", who);
  if (total == 0) return 0;
  const carl::AdamArgs a = carl_host::adam_args(ad);
  hipLaunchKernelGGL(carl::adam_step_sets_kernel, dim3(n_sets), dim3(carl::kAdamThreads), 0, (hipStream_t)stream, a, hyper);
  return check_launch(who);
}

}  // extern "C"
