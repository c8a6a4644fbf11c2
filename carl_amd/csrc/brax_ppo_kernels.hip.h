// brax_ppo_kernels.hip.h -- the PPO update of the Brax families on the device (include/carl_amd.h:
// carl_brax_policy_context_trace, carl_brax_ppo_grad).  Included by carl_brax_ppo.hip only.  Everything the classic unit
// has is called, not restated: ppo_device.hip.h's tile helpers (ppo_put, ppo_accumulate, ppo_accumulate_row,
// ppo_block_sum, ppo_act_grad, ppo_slab_index / ppo_slab_sum), policy_kernels.hip.h's dense_layer / head_layer / activate /
// normalize_input.  The CRITIC (one output, the same dense rows, the same input gather) is ppo_net_kernel<H> as it is
// (ppo_net_kernel.hip.h, instantiated by ppo_host.hpp's launch_ppo_net); the trace runs carl_ppo.hip's
// context_trace_kernel through launch_context_trace.  No kernel of another unit changes
// (profiles/brax_ppo_isa_identity.txt).
//
// What is new is the ACTOR's kernel, brax_ppo_actor_kernel<H>: ppo_net_kernel's scheme -- one persistent launch, the
// network staged in LDS once per workgroup, one sample per thread with its forward and backward pass in registers, a
// tile's activations and deltas through the two 260-float-pitch tile buffers, a fixed block of every dW per thread summed
// in sample order in blocks of 16, one slab per workgroup -- with a joint Gaussian head of up to kBraxPpoOut = 8 outputs.
//
// LDS (floats): the network  W1 [H][K] | b1 [H] | W2 [H][H] | b2 [H] | WhA^T [HI][4] | WhB^T [HI][4] | bh [8] | ls [8]
//               two tile buffers A, B [max(H, K)][kPpoPitch]
//               the head rows hd [16][kPpoPitch]: dy_j (rows 0 - 7), then the samples' dL/dlog_std_j terms (rows 8 - 15)
// The head is stored as two transposed halves of four outputs (actuators 0 - 3, 4 - 7), so that the forward pass is two
// head_layer calls; `ls` holds no parameter, it is the slab's place for the eight log_std gradients, which are column
// sums of head rows exactly as the head's bias gradients are.
// At H = 0 / 32 the head rows are a region of their own: 1 088 + 66 560 + 16 640 = 84 288 B (H = 0), 9 536 + 66 560 +
// 16 640 = 92 736 B (H = 32).  At H = 64 they do not fit behind the tile buffers (27 200 + 133 120 + 16 640 = 176 960 B of
// 163 840), and they live in rows [K, K + 16) = [32, 48) of B: those rows are dead from the moment the sample's inputs
// are in registers (the x rows are [0, 32)) until B takes h1 for the second layer's dW, which is behind the barrier that
// ends the head's reads.  27 200 + 133 120 = 160 320 B.
//
// Ownership of the head's gradients: thread tid owns dWh^T[j][k] for k = tid / 32 and the HI / 32 consecutive j from
// (tid % 32) * HI / 32 -- two entries at H = 64, one otherwise, every thread busy; threads 0 - 15 own dbh [8] and
// dlog_std [8] (head row tid).
#pragma once

#include "ppo_device.hip.h"

namespace carl {

constexpr int kBraxPpoOut = 8;             // head outputs the layout holds (the closed loop's limit on actuators)
constexpr int kBraxPpoHeadRows = 2 * kBraxPpoOut;

struct BraxPpoOffsets {
  int HI, kB1, kW2, kB2, kWh, kBh, kLs, kNet;
};
// (the sections below the head are ppo_offsets': ppo_slab_index serves them)
__host__ __device__ constexpr BraxPpoOffsets brax_ppo_offsets(int H) {
  const PpoOffsets o = ppo_offsets(H);
  const int kBh = o.kWh + o.HI * kBraxPpoOut;
  return BraxPpoOffsets{o.HI, o.kB1, o.kW2, o.kB2, o.kWh, kBh, kBh + kBraxPpoOut, kBh + 2 * kBraxPpoOut};
}
// whether the head rows live in rows [K, K + 16) of tile buffer B (header comment)
__host__ __device__ constexpr bool brax_ppo_head_in_b(int H) { return ppo_buf_rows(H) >= kPpoK + kBraxPpoHeadRows; }
__host__ __device__ constexpr size_t brax_ppo_lds_bytes(int H) {
  return ((size_t)brax_ppo_offsets(H).kNet + (size_t)2 * ppo_buf_rows(H) * kPpoPitch +
          (brax_ppo_head_in_b(H) ? 0 : (size_t)kBraxPpoHeadRows * kPpoPitch)) * sizeof(float);
}
__host__ __device__ constexpr int brax_ppo_slab_floats(int H) { return brax_ppo_offsets(H).kNet + kPpoStatFloats; }

// slab / LDS index of packed parameter e < weight_floats of the actor `s` at padded width H
__host__ __device__ inline int brax_ppo_slab_index(int H, const PpoShape& s, int e) {
  const BraxPpoOffsets o = brax_ppo_offsets(H);
  const int top = s.n_hidden == 0 ? s.n_in : s.n_hidden == 1 ? s.w0 : s.w1;
  const int head = s.weight_floats - s.n_out * (top + 1);  // the head's W [n_out][top], then its b
  if (e < head) return ppo_slab_index(H, s, e);
  e -= head;
  const int nw = s.n_out * top;
  if (e >= nw) return o.kBh + (e - nw);
  const int k = e / top, j = e % top;
  return o.kWh + (k / 4) * 4 * o.HI + 4 * j + k % 4;
}

// Preconditions (host, carl_brax_ppo.hip): the batch and the actor validated (dense rows: b.row_pitch == b.n_lanes;
// n_out <= kBraxPpoOut; the action column float32 [T][n_lanes][n_out]); H the actor's padded width; gridDim.x <= n_tiles;
// the dynamic LDS is brax_ppo_lds_bytes(H).  a.kind is not read; a.log_std: [n_out].
template <int H>
__global__ void __launch_bounds__(kPpoThreads) brax_ppo_actor_kernel(const PpoNetArgs a) {
  constexpr BraxPpoOffsets O = brax_ppo_offsets(H);
  constexpr int K = kPpoK;
  constexpr int NO = kBraxPpoOut;
  constexpr int HT = H == 0 ? 4 : H;
  constexpr int RI = H == 0 ? 1 : H / 16;
  constexpr int CH = O.HI / 32;  // entries of dWh^T a thread owns
  static_assert(O.HI % 32 == 0 && kPpoThreads == 32 * NO, "the head's ownership rule");
  extern __shared__ __attribute__((aligned(16))) float brax_ppo_lds[];
  float* const wts = brax_ppo_lds;
  float* const bufA = wts + O.kNet;
  float* const bufB = bufA + ppo_buf_rows(H) * kPpoPitch;
  float* const hd = brax_ppo_head_in_b(H) ? bufB + K * kPpoPitch : bufB + ppo_buf_rows(H) * kPpoPitch;
  const int tid = (int)threadIdx.x;
  const PpoShape& sh = a.shape;
  const int n_in = sh.n_in, n_out = sh.n_out, n_hidden = sh.n_hidden, act = sh.act;

  for (int e = tid; e < O.kNet; e += kPpoThreads) wts[e] = 0.0f;
  __syncthreads();
  for (int e = tid; e < sh.weight_floats; e += kPpoThreads) wts[brax_ppo_slab_index(H, sh, e)] = a.params[e];
  // rows of the tile buffers no sample writes stay zero for the whole launch (x rows >= n_in)
  for (int e = tid; e < (int)(brax_ppo_lds_bytes(H) / sizeof(float)) - O.kNet; e += kPpoThreads) bufA[e] = 0.0f;
  __syncthreads();

  const carl_ppo_batch_t& b = a.b;
  const size_t pitch = (size_t)b.row_pitch;
  const long long n_flat = (long long)b.n_steps * b.row_pitch;
  const float* const shift = a.xform;
  const float* const scale = a.xform + n_in;
  const float clip = a.xform[2 * n_in];
  const float c_lo = 1.0f - b.clip_range, c_hi = 1.0f + b.clip_range;
  float adv_mean = 0.0f, adv_rstd = 1.0f;
  if (b.adv_norm != nullptr) adv_mean = b.adv_norm[0], adv_rstd = b.adv_norm[1];
  const int bi = tid / 16, bj = tid % 16;
  float acc_w2[RI][RI], acc_w1[RI][2];
#pragma unroll
  for (int r = 0; r < RI; ++r) {
#pragma unroll
    for (int c = 0; c < RI; ++c) acc_w2[r][c] = 0.0f;
    acc_w1[r][0] = acc_w1[r][1] = 0.0f;
  }
  float acc_wh[1][CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) acc_wh[0][c] = 0.0f;
  float acc_b1 = 0.0f, acc_b2 = 0.0f, acc_hd = 0.0f;  // acc_hd: dbh (threads 0 - 7), dlog_std (threads 8 - 15)
  const int hk = tid / 32, hj = CH * (tid % 32);
  double st_pl = 0.0, st_ent = 0.0, st_kl = 0.0, st_clip = 0.0;

#pragma unroll 1
  for (int tile = (int)blockIdx.x; tile < a.n_tiles; tile += (int)gridDim.x) {
    const int m = tile * kPpoTile + tid;
    bool valid = m < b.n_samples;
    long long flat = 0;
    int t = 0, lane = 0;
    if (valid) {
      if (b.idx != nullptr) {
        flat = b.idx[m];
        valid = flat >= 0 && flat < n_flat;
        t = valid ? (int)(flat / b.row_pitch) : 0;
        lane = valid ? (int)(flat - (long long)t * b.row_pitch) : 0;
        valid = valid && lane < b.n_lanes;
      } else {
        t = m / b.n_lanes;
        lane = m - t * b.n_lanes;
        flat = (long long)t * b.row_pitch + lane;
      }
    }
    // the sample's input into rows [0, n_in) of this thread's column of B, as ppo_net_kernel stages it (rows [n_in, K)
    // hold zeros at the top of a tile).  Where there are hidden layers it is gathered a SECOND time for the first layer's
    // dW instead of being kept: 32 registers less all through the forward and the backward pass, which the H = 64
    // instance does not have (the same loads, the same arithmetic, the same bits).
    auto stage_x = [&]() {
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
    };
    stage_x();
    float x[K];
#pragma unroll
    for (int i = 0; i < K; ++i) x[i] = bufB[i * kPpoPitch + tid];
    // (the widths and the weights' offset opaque to the optimiser: ppo_net_kernel's comment)
    int w0 = sh.w0, w1 = sh.w1, woff = 0;
    asm volatile("" : "+s"(w0), "+s"(w1), "+s"(woff));
    const float* const w = wts + woff;
    float ya[4], yb[4];  // the head's outputs 0 - 3, 4 - 7
    [[maybe_unused]] float h1[HT], top[HT];
    if constexpr (H == 0) {
      head_layer<K>(w + O.kWh, w + O.kBh, x, ya);
      head_layer<K>(w + O.kWh + 4 * O.HI, w + O.kBh + 4, x, yb);
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
      head_layer<H>(w + O.kWh, w + O.kBh, top, ya);
      // (a scheduling fence: without it the second half's H weight reads are issued beside the first half's, 8 H registers
      // at once, and the H = 64 instance spills)
      asm volatile("" ::: "memory");
      head_layer<H>(w + O.kWh + 4 * O.HI, w + O.kBh + 4, top, yb);
    }

    // loss terms, dL/dy and the dL/dlog_std terms of this sample (not yet divided by n_samples)
    float dy[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) dy[j] = 0.0f;
    if (valid) {
#pragma clang fp contract(off)
      const float* const arow = static_cast<const float*>(b.action) + (size_t)flat * n_out;
      float z[NO];
      float lp = 0.0f, ent = 0.0f;
#pragma unroll
      for (int j = 0; j < NO; ++j) {
        z[j] = 0.0f;
        if (j < n_out) {  // (uniform)
          const float ls = a.log_std[j];
          const float inv_std = expf(-ls);
          z[j] = (arow[j] - (j < 4 ? ya[j & 3] : yb[j & 3])) * inv_std;
          const float lpj = __fmaf_rn(-0.5f * z[j], z[j], -ls - 0.918938533204672742f);
          const float ej = 1.418938533204672742f + ls;
          lp = j == 0 ? lpj : lp + lpj;
          ent = j == 0 ? ej : ent + ej;
          dy[j] = z[j] * inv_std;
        }
      }
      const float adv = b.adv_norm != nullptr ? (b.advantage[flat] - adv_mean) * adv_rstd : b.advantage[flat];
      const float lr = lp - b.log_prob[flat];
      const float r = expf(lr);
      const float rc = fminf(fmaxf(r, c_lo), c_hi);
      st_pl -= (double)fminf(r * adv, rc * adv);
      st_ent += (double)ent;
      st_kl += (double)((r - 1.0f) - lr);
      st_clip += fabsf(r - 1.0f) > b.clip_range ? 1.0 : 0.0;
      const bool clipped = (adv > 0.0f && r > c_hi) || (adv < 0.0f && r < c_lo);
      const float g = clipped ? 0.0f : -(adv * r);  // dL/dlp
#pragma unroll
      for (int j = 0; j < NO; ++j) {
        dy[j] = g * dy[j];
        ppo_put(hd, NO + j, j < n_out ? g * (z[j] * z[j] - 1.0f) - b.ent_coef : 0.0f);
      }
      if (a.new_out != nullptr) a.new_out[m] = lp;
    } else {
#pragma unroll
      for (int j = 0; j < NO; ++j) ppo_put(hd, NO + j, 0.0f);
    }

    // ---- backward: the head
#pragma unroll
    for (int j = 0; j < NO; ++j) ppo_put(hd, j, dy[j]);
    if constexpr (H == 0) {
#pragma unroll
      for (int i = 0; i < K; ++i) ppo_put(bufA, i, x[i]);
    } else {
#pragma unroll
      for (int j = 0; j < H; ++j) ppo_put(bufA, j, top[j]);
    }
    __syncthreads();
    ppo_accumulate<1, CH>(hd, hk, bufA, hj, acc_wh);
    if (tid < kBraxPpoHeadRows) ppo_accumulate_row(hd, tid, acc_hd);
    if constexpr (H > 0) {
      // (the backward pass reads the weights through an offset of its own: ppo_net_kernel's comment)
      int boff = 0;
      asm volatile("" : "+s"(boff));
      const float* const wb = wts + boff;
      // deltas of the last hidden layer: (Wh^T dy) * act', actuators in order
#pragma unroll
      for (int j = 0; j < H; ++j) {
        if (j % 16 == 0) asm volatile("" ::: "memory");  // (the same fence: at most 16 rows' weight reads in flight)
        const pvf4 wa = bcast4(wb + O.kWh + 4 * j);
        const pvf4 wc = bcast4(wb + O.kWh + 4 * O.HI + 4 * j);
        float g = wa.x * dy[0];
        g = __fmaf_rn(wa.y, dy[1], g);
        g = __fmaf_rn(wa.z, dy[2], g);
        g = __fmaf_rn(wa.w, dy[3], g);
        g = __fmaf_rn(wc.x, dy[4], g);
        g = __fmaf_rn(wc.y, dy[5], g);
        g = __fmaf_rn(wc.z, dy[6], g);
        g = __fmaf_rn(wc.w, dy[7], g);
        top[j] = g * ppo_act_grad(top[j], act);
      }
      __syncthreads();  // (every read of A and of the head rows is done)
      if (n_hidden > 1) {  // (uniform)
#pragma unroll
        for (int j = 0; j < H; ++j) {
          ppo_put(bufA, j, top[j]);
          ppo_put(bufB, j, h1[j]);
        }
        __syncthreads();
        ppo_accumulate<RI, RI>(bufA, RI * bi, bufB, RI * bj, acc_w2);
        if (tid < H) ppo_accumulate_row(bufA, tid, acc_b2);
        // deltas of the first hidden layer: (W2^T d2) * act' (a real loop over the rows: ppo_net_kernel's comment)
        float d1[H];
#pragma unroll
        for (int i = 0; i < H; ++i) d1[i] = 0.0f;
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
      stage_x();
#pragma unroll 1
      for (int i = n_in; i < K; ++i) ppo_put(bufB, i, 0.0f);
      __syncthreads();
      ppo_accumulate<RI, 2>(bufA, RI * bi, bufB, 2 * bj, acc_w1);
      if (tid < H) ppo_accumulate_row(bufA, tid, acc_b1);
    }
    __syncthreads();  // (the next tile writes A / B / the head rows)
  }

  // ---- this workgroup's slab
  float* const slab = a.slab + (size_t)blockIdx.x * brax_ppo_slab_floats(H);
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
#pragma unroll
  for (int c = 0; c < CH; ++c) slab[O.kWh + (hk / 4) * 4 * O.HI + 4 * (hj + c) + hk % 4] = acc_wh[0][c];
  if (tid < kBraxPpoHeadRows) slab[O.kBh + tid] = acc_hd;  // (kLs = kBh + 8)
  double* const red = reinterpret_cast<double*>(bufA);
  const double sums[4] = {st_pl, st_ent, st_kl, st_clip};
  for (int q = 0; q < 4; ++q) {
    const double s = ppo_block_sum(red, sums[q]);
    if (tid == 0) slab[O.kNet + q] = (float)s;
  }
  if (tid < 4) slab[O.kNet + 4 + tid] = 0.0f;
}

// One thread per output: the packed gradient entries of the actor (its slabs in this unit's layout), then of the critic
// (ppo_net_kernel's slabs), then the 6 statistics and the n_out entries of grad_log_std.  PpoReduceArgs as
// ppo_reduce_kernel reads it; every sum is a fixed function of the slabs.
__global__ void __launch_bounds__(256) brax_ppo_reduce_kernel(const PpoReduceArgs a) {
  const int n_a = a.actor.set_floats, n_c = a.critic.set_floats;
  const int sa = brax_ppo_slab_floats(a.h_actor), sc = ppo_slab_floats(a.h_critic);
  const BraxPpoOffsets oa = brax_ppo_offsets(a.h_actor);
  const int kc = ppo_offsets(a.h_critic).kNet;
  const int n_extra = 6 + kBraxPpoOut;
  for (int e = (int)(blockIdx.x * blockDim.x + threadIdx.x); e < n_a + n_c + n_extra; e += (int)(gridDim.x * blockDim.x)) {
    if (e < n_a) {
      a.grad_actor[e] = e < a.actor.weight_floats
          ? (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, brax_ppo_slab_index(a.h_actor, a.actor, e)) * a.inv_m) : 0.0f;
    } else if (e < n_a + n_c) {
      const int k = e - n_a;
      a.grad_critic[k] = k < a.critic.weight_floats
          ? (float)(ppo_slab_sum(a.slab_critic, sc, a.n_workgroups, ppo_slab_index(a.h_critic, a.critic, k)) * a.inv_m) : 0.0f;
    } else {
      const int q = e - n_a - n_c;
      if (q < 4) a.stats[q == 0 ? 0 : q + 1] = (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, oa.kNet + q) * a.inv_m);
      else if (q == 4) a.stats[1] = (float)(ppo_slab_sum(a.slab_critic, sc, a.n_workgroups, kc + 4) * a.inv_m);
      else if (q == 5) a.stats[5] = a.n_samples;
      else if (q - 6 < a.actor.n_out)
        a.grad_log_std[q - 6] = (float)(ppo_slab_sum(a.slab_actor, sa, a.n_workgroups, oa.kLs + (q - 6)) * a.inv_m);
    }
  }
}

}  // namespace carl
