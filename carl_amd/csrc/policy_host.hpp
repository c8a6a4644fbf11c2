// policy_host.hpp -- host-side rules of the closed-loop rollout, shared by its four translation units: the shapes of a
// packed network and the checks of the deterministic entry points (defined in carl_policy.hip), the sampling checks
// (carl_policy_sample.hip).  Each check and its message is written once; the launch path is policy_launch.hpp's.
#pragma once

#include <cstdint>

#include "../../include/carl_amd.h"

namespace carl_host {
// floats of one packed weight set (include/carl_amd.h), or -1 for a shape outside the limits
int policy_set_floats(const carl_policy_t* p);
// floats of a packed weight set before its shift | scale | clip section (every W and b); the shape is a valid one
int policy_transform_offset(const carl_policy_t* p);
// the instantiated hidden width a policy is padded to: 0 (a linear policy), 32, 64
int policy_padded_hidden(const carl_policy_t* p);

// What every packed network is checked for, the actor (by check_rollout_policy / check_evaluate_policy) and the critic
// (carl_policy_value.hip, with a `who` of "<entry point>: critic"): n_hidden and width[] in range, a known activation,
// params not NULL.  Three functions, because each caller has checks of its own between them.
int check_hidden_layers(const char* who, const carl_policy_t* p);
int check_activation(const char* who, const carl_policy_t* p);
int check_params(const char* who, const carl_policy_t* p);

// Every check of carl_rollout_policy / carl_evaluate_policy, in its order, with messages that begin with `who`; 0 when
// the call may go on, `fi` then holds the batch family's info.
int check_rollout_policy(const char* who, const carl_batch_t* batch, const carl_policy_t* policy, const carl_step_io_t* io,
                         int32_t n_steps, const carl_policy_summary_t* summary_out, carl_family_info_t* fi);
int check_evaluate_policy(const char* who, const carl_batch_t* batch, const carl_policy_t* policy, int32_t n_episodes,
                          int32_t max_steps, const carl_policy_episodes_t* out, carl_family_info_t* fi);
// what a sampled launch refuses on top of its deterministic twin's checks (defined in carl_policy_sample.hip).
// log_prob: refused where the mode stores no per-step column, required by the launch with a critic
enum class LogProb { kRefused, kOptional, kRequired };
int check_sampling(const char* who, const carl_policy_sampling_t* smp, const carl_family_info_t& fi, LogProb log_prob);
// a validated rollout without a step (n_lanes == 0 or n_steps == 0): zero the summary totals, if any
int policy_rollout_without_steps(const char* who, const carl_batch_t* batch, const carl_policy_summary_t* summary_out,
                                 void* stream);
// the statistics output of an episodes launch that gathers input statistics, or of their merge (defined in
// carl_policy_stats.hip): stats and stats->partial not NULL, partial on a 16-byte boundary, room for n_slabs slabs.
// `slabs`: what a slab is called and which function counts them, for the message
int check_policy_stats(const char* who, const carl_policy_stats_t* stats, int n_slabs, const char* slabs);
}  // namespace carl_host
