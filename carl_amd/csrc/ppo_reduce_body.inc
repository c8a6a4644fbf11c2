// ppo_reduce_body.inc -- the body of ppo_reduce_kernel (ppo_kernels.hip.h) and of the population's reduction
// (ppo_sets_kernels.hip.h: ppo_reduce_sets_kernel), included textually inside each, as ppo_net_body.inc is.  In scope: `a`,
// the PpoReduceArgs of ONE learner.  One thread per output: the packed gradient entries of the actor, then of the critic,
// then the 6 statistics and grad_log_std; blockIdx.x / gridDim.x are of one learner's launch shape.  Every sum is a fixed
// function of the slabs.
  const int n_a = a.actor.set_floats, n_c = a.critic.set_floats;
  const int sa = ppo_slab_floats(a.h_actor), sc = ppo_slab_floats(a.h_critic);
  const int ka = ppo_offsets(a.h_actor).kNet, kc = ppo_offsets(a.h_critic).kNet;
  for (int e = (int)(blockIdx.x * blockDim.x + threadIdx.x); e < n_a + n_c + 8; e += (int)(gridDim.x * blockDim.x)) {
    if (e < n_a) {
      a.grad_actor[e] = e < a.actor.weight_floats
          ? (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, ppo_slab_index(a.h_actor, a.actor, e)) * a.inv_m) : 0.0f;
    } else if (e < n_a + n_c) {
      const int k = e - n_a;
      a.grad_critic[k] = k < a.critic.weight_floats
          ? (float)(ppo_slab_sum(a.slab_critic, sc, a.n_workgroups, ppo_slab_index(a.h_critic, a.critic, k)) * a.inv_m) : 0.0f;
    } else {
      const int q = e - n_a - n_c;
      if (q < 4) a.stats[q == 0 ? 0 : q + 1] = (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, ka + q) * a.inv_m);
      else if (q == 4) a.stats[1] = (float)(ppo_slab_sum(a.slab_critic, sc, a.n_workgroups, kc + 4) * a.inv_m);
      else if (q == 5) a.stats[5] = a.n_samples;
      else if (q == 6 && a.gaussian) a.grad_log_std[0] = (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, ka + 5) * a.inv_m);
    }
  }
