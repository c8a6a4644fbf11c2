// ppo_net_body.inc -- the body of ppo_net_kernel<H> (ppo_net_kernel.hip.h) and of the population kernel
// ppo_net_sets_kernel<H> (ppo_sets_kernels.hip.h), included textually inside each, as policy_rollout_body.inc is: the
// compiler sees every kernel's arguments as kernel arguments.  What a workgroup reads per LEARNER rather than per launch
// stands here as a macro the including kernel defines: PPO_MB_PARAMS, PPO_MB_XFORM, PPO_MB_LOG_STD, PPO_MB_SLAB,
// PPO_MB_NEW_OUT, PPO_MB_IDX, PPO_MB_ADV_NORM (pointers), PPO_MB_CLIP_RANGE, PPO_MB_VF_COEF, PPO_MB_ENT_COEF (floats).  The
// one-set kernel defines each as the argument expression that stood in its place (a.params, a.b.idx, ...), so it compiles
// to exactly the code it had (profiles/ppo_sets_refactor_identity.txt; a local alias moves the kernel-argument loads); the
// population kernel defines them as its member's values.  PPO_MB_LANE_WINDOW (a constant expression) and, read only where
// it is true, PPO_MB_LANE_LO / PPO_MB_LANE_HI: a sample whose lane lies outside [LO, HI) then contributes zero, exactly like
// an index outside the buffer.  Otherwise in scope: H; `a`, the launch's PpoNetArgs.  blockIdx.x / gridDim.x are the
// workgroup and the workgroup count of ONE learner's launch shape.
  constexpr PpoOffsets O = ppo_offsets(H);
  constexpr int K = kPpoK;
  constexpr int HT = H == 0 ? 4 : H;  // (array sizes of the H == 0 instance, whose hidden code is discarded)
  constexpr int RI = H == 0 ? 1 : H / 16;  // rows / columns of a thread's block of dW2, rows of its block of dW1
  extern __shared__ __attribute__((aligned(16))) float ppo_lds[];
  float* const wts = ppo_lds;
  float* const bufA = wts + O.kNet;
  float* const bufB = bufA + ppo_buf_rows(H) * kPpoPitch;
  float* const dyb = bufB + ppo_buf_rows(H) * kPpoPitch;
  const int tid = (int)threadIdx.x;
  const PpoShape& sh = a.shape;
  const int n_in = sh.n_in, n_out = sh.n_out, n_hidden = sh.n_hidden, act = sh.act;

  // the network into LDS: zeros, then every packed parameter at its slot
  for (int e = tid; e < O.kNet; e += kPpoThreads) wts[e] = 0.0f;
  __syncthreads();
  for (int e = tid; e < sh.weight_floats; e += kPpoThreads) wts[ppo_slab_index(H, sh, e)] = PPO_MB_PARAMS[e];
  // rows of the tile buffers no sample writes stay zero for the whole launch (dy rows >= n_out; x rows >= n_in)
  for (int e = tid; e < 2 * ppo_buf_rows(H) * kPpoPitch + 4 * kPpoPitch; e += kPpoThreads) bufA[e] = 0.0f;
  __syncthreads();

  const carl_ppo_batch_t& b = a.b;
  const size_t pitch = (size_t)b.row_pitch;
  const long long n_flat = (long long)b.n_steps * b.row_pitch;
  const float* const shift = PPO_MB_XFORM;
  const float* const scale = PPO_MB_XFORM + n_in;
  const float clip = PPO_MB_XFORM[2 * n_in];
  const float c_lo = 1.0f - PPO_MB_CLIP_RANGE, c_hi = 1.0f + PPO_MB_CLIP_RANGE;
  float adv_mean = 0.0f, adv_rstd = 1.0f;
  if (PPO_MB_ADV_NORM != nullptr) adv_mean = PPO_MB_ADV_NORM[0], adv_rstd = PPO_MB_ADV_NORM[1];
  float ls = 0.0f, inv_std = 1.0f, lp0 = 0.0f;
  if (a.kind == kPpoGaussian) {
    ls = PPO_MB_LOG_STD[0];
    inv_std = expf(-ls);
    lp0 = -ls - 0.918938533204672742f;
  }
  // this thread's blocks of the weight gradients (header comment); the accumulators live across the tiles
  const int bi = tid / 16, bj = tid % 16;
  float acc_w2[RI][RI], acc_w1[RI][2];
#pragma unroll
  for (int r = 0; r < RI; ++r) {
#pragma unroll
    for (int c = 0; c < RI; ++c) acc_w2[r][c] = 0.0f;
    acc_w1[r][0] = acc_w1[r][1] = 0.0f;
  }
  float acc_wh[1][1] = {{0.0f}};  // dWh^T[j][k], k = tid / HI, j = tid % HI (threads below 4 HI)
  float acc_b1 = 0.0f, acc_b2 = 0.0f, acc_bh = 0.0f;
  const int hk = tid / O.HI, hj = tid % O.HI;
  double st_pl = 0.0, st_ent = 0.0, st_kl = 0.0, st_clip = 0.0, st_vl = 0.0, st_dls = 0.0;

#pragma unroll 1
  for (int tile = (int)blockIdx.x; tile < a.n_tiles; tile += (int)gridDim.x) {
    const int m = tile * kPpoTile + tid;
    bool valid = m < b.n_samples;
    long long flat = 0;
    int t = 0, lane = 0;
    if (valid) {
      if (PPO_MB_IDX != nullptr) {
        flat = PPO_MB_IDX[m];
        valid = flat >= 0 && flat < n_flat;
        t = valid ? (int)(flat / b.row_pitch) : 0;
        lane = valid ? (int)(flat - (long long)t * b.row_pitch) : 0;
        valid = valid && lane < b.n_lanes;
        if constexpr (PPO_MB_LANE_WINDOW) valid = valid && lane >= PPO_MB_LANE_LO && lane < PPO_MB_LANE_HI;
      } else {
        t = m / b.n_lanes;
        lane = m - t * b.n_lanes;
        flat = (long long)t * b.row_pitch + lane;
      }
    }
    // the sample's input, as the rollout's actor saw it; an invalid sample runs on zeros and contributes zeros.  The
    // n_in real inputs go through this thread's column of B (a runtime loop: no per-slot masks); rows [n_in, K) of B
    // hold zeros here (the initial fill, then the x rows the previous tile wrote last).
    if (valid) {
      const int c = min(max(b.context_id[flat], 0), b.n_contexts - 1);
      const float* const o = (t == 0 ? b.obs0 + (size_t)lane * b.obs_dim
                                     : b.obs + ((size_t)(t - 1) * pitch + lane) * b.obs_dim) - a.n_ctx;
#pragma unroll 1
      for (int i = 0; i < n_in; ++i) {
        const float v = i < a.n_ctx ? b.ctx_table[(size_t)a.ctx_rows[i] * b.ctx_stride + c] : o[i];
        ppo_put(bufB, i, normalize_input(v, shift[i], scale[i], clip));
      }
    } else {
#pragma unroll 1
      for (int i = 0; i < n_in; ++i) ppo_put(bufB, i, 0.0f);
    }
    float x[K];
#pragma unroll
    for (int i = 0; i < K; ++i) x[i] = bufB[i * kPpoPitch + tid];
    // The layer widths and the weights' offset, opaque to the optimiser from here on: the widths as in
    // policy_value_kernels.hip.h (the padded units' masks); the offset so that the weight reads of a tile are not all
    // hoisted above the tile loop (they are loop-invariant: thousands of registers, spilled)
    int w0 = sh.w0, w1 = sh.w1, woff = 0;
    asm volatile("" : "+s"(w0), "+s"(w1), "+s"(woff));
    const float* const w = wts + woff;
    float y[4];
    [[maybe_unused]] float h1[HT], top[HT];  // top: the last hidden layer's activations, then its deltas
    if constexpr (H == 0) {
      head_layer<K>(w + O.kWh, w + O.kBh, x, y);
    } else {
      dense_layer<H, K>(w, w + O.kB1, x, h1);
      activate(h1, act, w0);
      if (n_hidden > 1) {  // (uniform)
        dense_layer<H, H>(w + O.kW2, w + O.kB2, h1, top);
        activate(top, act, w1);
      } else {
#pragma unroll
        for (int j = 0; j < H; ++j) top[j] = h1[j];
      }
      head_layer<H>(w + O.kWh, w + O.kBh, top, y);
    }

    // loss terms and dL/dy of this sample (not yet divided by n_samples)
    float dy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
#pragma clang fp contract(off)
      if (a.kind == kPpoValue) {
        const float v = y[0], ret = b.ret[flat];
        const float d = ret - v;
        st_vl += (double)(d * d);
        dy[0] = PPO_MB_VF_COEF * (2.0f * (v - ret));
        if (PPO_MB_NEW_OUT != nullptr) PPO_MB_NEW_OUT[m] = v;
      } else {
        float lp, ent;
        float p[4] = {0.0f, 0.0f, 0.0f, 0.0f}, logp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int ai = 0;
        float z = 0.0f;
        if (a.kind == kPpoCategorical) {
          ai = min(max(static_cast<const int*>(b.action)[flat], 0), n_out - 1);
          float mx = y[0];
#pragma unroll
          for (int k = 1; k < 4; ++k) mx = k < n_out ? fmaxf(mx, y[k]) : mx;
          float e[4], s = 0.0f;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            e[k] = k < n_out ? expf(y[k] - mx) : 0.0f;
            s = k < n_out ? s + e[k] : s;
          }
          const float log_s = logf(s);
          ent = 0.0f;
          float ya = y[0];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k < n_out) {
              p[k] = e[k] / s;
              logp[k] = (y[k] - mx) - log_s;
              ent -= p[k] * logp[k];
            }
            ya = k == ai ? y[k] : ya;
          }
          lp = (ya - mx) - log_s;
        } else {
          z = (static_cast<const float*>(b.action)[flat] - y[0]) * inv_std;
          lp = __fmaf_rn(-0.5f * z, z, lp0);
          ent = 1.418938533204672742f + ls;
        }
        const float adv = PPO_MB_ADV_NORM != nullptr ? (b.advantage[flat] - adv_mean) * adv_rstd : b.advantage[flat];
        const float lr = lp - b.log_prob[flat];
        const float r = expf(lr);
        const float rc = fminf(fmaxf(r, c_lo), c_hi);
        st_pl -= (double)fminf(r * adv, rc * adv);
        st_ent += (double)ent;
        st_kl += (double)((r - 1.0f) - lr);
        st_clip += fabsf(r - 1.0f) > PPO_MB_CLIP_RANGE ? 1.0 : 0.0;
        const bool clipped = (adv > 0.0f && r > c_hi) || (adv < 0.0f && r < c_lo);
        const float g = clipped ? 0.0f : -(adv * r);  // dL/dlp
        if (a.kind == kPpoCategorical) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < n_out) dy[k] = g * ((k == ai ? 1.0f : 0.0f) - p[k]) + PPO_MB_ENT_COEF * (p[k] * (logp[k] + ent));
        } else {
          dy[0] = g * (z * inv_std);
          st_dls += (double)(g * (z * z - 1.0f) - PPO_MB_ENT_COEF);
        }
        if (PPO_MB_NEW_OUT != nullptr) PPO_MB_NEW_OUT[m] = lp;
      }
    }

    // ---- backward: the head
#pragma unroll
    for (int k = 0; k < 4; ++k) ppo_put(dyb, k, dy[k]);
    if constexpr (H == 0) {
#pragma unroll
      for (int i = 0; i < K; ++i) ppo_put(bufA, i, x[i]);
    } else {
#pragma unroll
      for (int j = 0; j < H; ++j) ppo_put(bufA, j, top[j]);
    }
    __syncthreads();
    if (tid < 4 * O.HI) ppo_accumulate<1, 1>(dyb, hk, bufA, hj, acc_wh);
    if (tid < 4) ppo_accumulate_row(dyb, tid, acc_bh);
    if constexpr (H > 0) {
      // The backward pass reads the weights through an offset of its own: read through the forward pass's pointer, the
      // compiler keeps every weight the forward pass loaded alive for it (the same addresses: H * H registers, spilled).
      int boff = 0;
      asm volatile("" : "+s"(boff));
      const float* const wb = wts + boff;
      // deltas of the last hidden layer: (Wh^T dy) * act'
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const pvf4 ww = bcast4(wb + O.kWh + 4 * j);
        float g = ww.x * dy[0];
        g = __fmaf_rn(ww.y, dy[1], g);
        g = __fmaf_rn(ww.z, dy[2], g);
        g = __fmaf_rn(ww.w, dy[3], g);
        top[j] = g * ppo_act_grad(top[j], act);
      }
      __syncthreads();  // (every read of A is done)
      if (n_hidden > 1) {  // (uniform)
#pragma unroll
        for (int j = 0; j < H; ++j) {
          ppo_put(bufA, j, top[j]);
          ppo_put(bufB, j, h1[j]);
        }
        __syncthreads();
        ppo_accumulate<RI, RI>(bufA, RI * bi, bufB, RI * bj, acc_w2);
        if (tid < H) ppo_accumulate_row(bufA, tid, acc_b2);
        // deltas of the first hidden layer: (W2^T d2) * act', row j of W2 read as broadcasts
        float d1[H];
#pragma unroll
        for (int i = 0; i < H; ++i) d1[i] = 0.0f;
        // (a real loop over the rows, d2 re-read from this thread's column of A: unrolled, all H * H / 4 weight reads
        // are issued ahead of the first fma and spilled)
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
          const float dj = bufA[j * kPpoPitch + tid];
#pragma unroll
          for (int i = 0; i < H; i += 4) {
            const pvf4 ww = bcast4(wb + O.kW2 + j * H + i);
            d1[i] = __fmaf_rn(ww.x, dj, d1[i]);
            d1[i + 1] = __fmaf_rn(ww.y, dj, d1[i + 1]);
            d1[i + 2] = __fmaf_rn(ww.z, dj, d1[i + 2]);
            d1[i + 3] = __fmaf_rn(ww.w, dj, d1[i + 3]);
          }
        }
#pragma unroll
        for (int i = 0; i < H; ++i) top[i] = d1[i] * ppo_act_grad(h1[i], act);
        __syncthreads();
      }
      // ---- the first layer: top holds its deltas
#pragma unroll
      for (int j = 0; j < H; ++j) ppo_put(bufA, j, top[j]);
#pragma unroll
      for (int i = 0; i < K; ++i) ppo_put(bufB, i, x[i]);
      __syncthreads();
      ppo_accumulate<RI, 2>(bufA, RI * bi, bufB, 2 * bj, acc_w1);
      if (tid < H) ppo_accumulate_row(bufA, tid, acc_b1);
    }
    __syncthreads();  // (the next tile writes A / B / dy)
  }

  // ---- this workgroup's slab
  float* const slab = PPO_MB_SLAB + (size_t)blockIdx.x * ppo_slab_floats(H);
  if constexpr (H > 0) {
#pragma unroll
    for (int r = 0; r < RI; ++r) {
#pragma unroll
      for (int c = 0; c < RI; ++c) slab[O.kW2 + (RI * bi + r) * H + RI * bj + c] = acc_w2[r][c];
      slab[(RI * bi + r) * K + 2 * bj] = acc_w1[r][0];
      slab[(RI * bi + r) * K + 2 * bj + 1] = acc_w1[r][1];
    }
    if (tid < H) {
      slab[O.kB1 + tid] = acc_b1;
      slab[O.kB2 + tid] = acc_b2;
    }
  }
  if (tid < 4 * O.HI) slab[O.kWh + 4 * hj + hk] = acc_wh[0][0];
  if (tid < 4) slab[O.kBh + tid] = acc_bh;
  double* const red = reinterpret_cast<double*>(bufA);
  const double sums[6] = {st_pl, st_ent, st_kl, st_clip, st_vl, st_dls};
  for (int q = 0; q < 6; ++q) {
    const double s = ppo_block_sum(red, sums[q]);
    if (tid == 0) slab[O.kNet + q] = (float)s;
  }
  if (tid == 0) slab[O.kNet + 6] = slab[O.kNet + 7] = 0.0f;
