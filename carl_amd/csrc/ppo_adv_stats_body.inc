// ppo_adv_stats_body.inc -- the body of ppo_adv_stats_kernel (ppo_step_kernels.hip.h) and of the population kernel
// ppo_adv_stats_sets_kernel (ppo_sets_kernels.hip.h), included textually inside each, as ppo_net_body.inc is, behind the
// kernel's `#pragma clang fp contract(off)`.  In scope: `a`, the launch's PpoAdvStatsArgs; the macros ADV_MB_IDX, ONE
// learner's epoch [n_total], and ADV_MB_ADV_NORM, its rows [gridDim.x][2] (the one-set kernel: a.idx, a.adv_norm).
// Workgroup blockIdx.x takes minibatch blockIdx.x of that epoch.
  __shared__ double red[kAdvThreads / 64 + 1];
  const int tid = (int)threadIdx.x;
  const long long first = (long long)blockIdx.x * a.batch_size;
  const long long left = (long long)a.n_total - first;
  const int n = (int)(left < a.batch_size ? left : a.batch_size);  // >= 1
  const int32_t* const idx = ADV_MB_IDX + first;
  if (n == 1) {  // the identity: what passing no adv_norm does
    if (tid == 0) ADV_MB_ADV_NORM[(size_t)blockIdx.x * 2] = 0.0f, ADV_MB_ADV_NORM[(size_t)blockIdx.x * 2 + 1] = 1.0f;
    return;
  }
  const long long j0 = idx[0];
  const bool in0 = j0 >= 0 && j0 < a.storage_floats;
  const double c = in0 ? (double)a.advantage[j0] : 0.0;  // (an index outside the storage: the shift is 0)
  double s1 = 0.0, s2 = 0.0;
  // kAdvAhead of the thread's gathers are issued before the dependent float64 chain, as ppo_input_stats_kernel issues
  // its passes: a sample past the end or outside the storage loads element 0 (storage_floats >= 1) and adds nothing.
#pragma unroll 1
  for (int i0 = tid; i0 < n; i0 += kAdvAhead * kAdvThreads) {
    bool ok[kAdvAhead];
    long long j[kAdvAhead];
    float x[kAdvAhead];
#pragma unroll
    for (int k = 0; k < kAdvAhead; ++k) {
      const int i = i0 + k * kAdvThreads;
      j[k] = idx[i < n ? i : 0];
      ok[k] = i < n && j[k] >= 0 && j[k] < a.storage_floats;
    }
#pragma unroll
    for (int k = 0; k < kAdvAhead; ++k) x[k] = a.advantage[ok[k] ? j[k] : 0];
#pragma unroll
    for (int k = 0; k < kAdvAhead; ++k) {
      if (ok[k]) {
        const double d = (double)x[k] - c;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  const double S1 = step_block_sum<kAdvThreads>(red, s1);
  const double S2 = step_block_sum<kAdvThreads>(red, s2);
  if (tid == 0) {
    const double nn = (double)n;
    const double mean = c + S1 / nn;
    double var = (S2 - S1 * S1 / nn) / (nn - 1.0);
    var = var > 0.0 ? var : 0.0;
    ADV_MB_ADV_NORM[(size_t)blockIdx.x * 2] = (float)mean;
    ADV_MB_ADV_NORM[(size_t)blockIdx.x * 2 + 1] = (float)(1.0 / (sqrt(var) + a.eps));
  }
