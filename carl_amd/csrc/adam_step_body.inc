// adam_step_body.inc -- the body of adam_step_kernel (ppo_step_kernels.hip.h) and of the population kernel
// adam_step_sets_kernel (ppo_sets_kernels.hip.h), included textually inside each, as ppo_net_body.inc is, behind the kernel's
// `#pragma clang fp contract(off)`.  In scope: `a`, the launch's AdamArgs (its tensors' first rows, the shared betas and
// eps); and as macros what is ONE learner's: ADAM_MB_ROW(ptr, t), the learner's row of tensor t given its first row;
// ADAM_MB_STEP, ADAM_MB_BETA_POW, ADAM_MB_NORM_OUT (pointers to its state); ADAM_MB_LR, ADAM_MB_MAX_GRAD_NORM (doubles).
// The one-set kernel defines them as the arguments that stood in their place.  One workgroup, one learner.
  __shared__ double red[kAdamThreads / 64 + 1];
  const int tid = (int)threadIdx.x;
  // every thread reads the state before the sum's barriers; thread 0 writes it behind them
  const int64_t step = ADAM_MB_STEP[0];
  const double bp1 = ADAM_MB_BETA_POW[0] * a.beta1, bp2 = ADAM_MB_BETA_POW[1] * a.beta2;
  double s = 0.0;
  for (int t = 0; t < a.n_tensors; ++t) {
    const float* const g = ADAM_MB_ROW(a.grad[t], t);
    const long long n = a.n[t];
#pragma unroll 1
    for (long long i0 = tid; i0 < n; i0 += (long long)kAdamAhead * kAdamThreads) {
      float x[kAdamAhead];
#pragma unroll
      for (int k = 0; k < kAdamAhead; ++k) {
        const long long i = i0 + (long long)k * kAdamThreads;
        x[k] = i < n ? g[i] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < kAdamAhead; ++k) {
        const double d = (double)x[k];
        s += d * d;  // (a slot past the end adds +0.0 to a sum that is never -0.0)
      }
    }
  }
  const double norm = sqrt(step_block_sum<kAdamThreads>(red, s));
  const double ratio = ADAM_MB_MAX_GRAD_NORM / (norm + 1e-6);  // (+inf: no clip)
  const double coef = ratio < 1.0 ? ratio : 1.0;
  if (tid == 0) {
    ADAM_MB_STEP[0] = step + 1;
    ADAM_MB_BETA_POW[0] = bp1;
    ADAM_MB_BETA_POW[1] = bp2;
    if (ADAM_MB_NORM_OUT != nullptr) ADAM_MB_NORM_OUT[0] = norm, ADAM_MB_NORM_OUT[1] = coef;
  }
  const double omb1 = 1.0 - a.beta1, omb2 = 1.0 - a.beta2;
  const double step_size = ADAM_MB_LR / (1.0 - bp1), sqrt_bc2 = sqrt(1.0 - bp2);
  for (int t = 0; t < a.n_tensors; ++t) {
    const float* const g = ADAM_MB_ROW(a.grad[t], t);
    float* const p = ADAM_MB_ROW(a.param[t], t);
    float* const m = ADAM_MB_ROW(a.m[t], t);
    float* const v = ADAM_MB_ROW(a.v[t], t);
    const long long n = a.n[t];
    for (long long i = tid; i < n; i += kAdamThreads) {
      const double gd = (double)g[i] * coef;
      const float mf = (float)(a.beta1 * (double)m[i] + omb1 * gd);
      const float vf = (float)(a.beta2 * (double)v[i] + omb2 * gd * gd);
      m[i] = mf;
      v[i] = vf;
      p[i] = (float)((double)p[i] - step_size * (double)mf / (sqrt((double)vf) / sqrt_bc2 + a.eps));
    }
  }
