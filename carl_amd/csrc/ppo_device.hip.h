// ppo_device.hip.h -- what the kernels of the PPO update on the device share (ppo_net_kernel.hip.h, ppo_kernels.hip.h,
// brax_ppo_kernels.hip.h): the LDS / slab layout of a network, the kernels' argument structs and the tile helpers.  No
// kernel is defined here.  The device functions of policy_kernels.hip.h
// (bcast4, dense_layer, head_layer, activate, normalize_input) are called, none is changed.
//
// LDS (floats): the network  W1 [H][K] | b1 [H] | W2 [H][H] | b2 [H] | Wh^T [HI][4] | bh [4]   (HI = H ? H : K)
//               two tile buffers A, B [max(H, K)][kPpoPitch]  (row = unit, column = sample of the tile)
//               dy [4][kPpoPitch]
// At H = 64: 26 128 + 2 x 66 560 + 4 160 = 163 408 bytes of the 163 840 a compute unit has -- which is why the actor
// and the critic are two launches.  A tile buffer is written by the sample's thread (column s: consecutive lanes,
// consecutive banks) and read along s as float4 by the accumulating threads; the pitch of 260 floats shifts row j by
// 4 j banks, so the 16 rows a wavefront reads at once cover the 64 banks.
//
// Between the layers of the backward pass a tile's activations and deltas go through A / B and every thread adds
//   dW[i][j] += sum_s delta[s][i] * h[s][j]
// for its own fixed block of (i, j), s in index order in blocks of 16 (fma chain inside a block, the block sums added
// in order, the tile sum added to the accumulator that lives in registers across the workgroup's tiles).  At the end a
// workgroup writes its accumulators as one slab in the LDS layout above, plus 8 floats of loss statistics; a reduction
// kernel adds the slabs in workgroup order in float64.
#pragma once

#include "policy_kernels.hip.h"

namespace carl {

constexpr int kPpoThreads = 256;
constexpr int kPpoTile = kPpoThreads;       // samples per tile: one per thread
constexpr int kPpoK = CARL_POLICY_MAX_IN;   // input slots
constexpr int kPpoPitch = kPpoTile + 4;     // floats per row of a tile buffer
constexpr int kPpoMaxWorkgroups = 256;      // one per compute unit; the partial slabs stay below 7 MB per network
constexpr int kPpoStatFloats = 8;           // per slab: pl, entropy, kl, clipped, vl, dlog_std, -, - (sums)
enum { kPpoCategorical = 0, kPpoGaussian = 1, kPpoValue = 2 };

// offsets of the LDS / slab layout of a network at padded width H
struct PpoOffsets {
  int HI, kB1, kW2, kB2, kWh, kBh, kNet;
};
__host__ __device__ constexpr PpoOffsets ppo_offsets(int H) {
  const int HI = H == 0 ? kPpoK : H;
  const int kB1 = H * kPpoK, kW2 = kB1 + H, kB2 = kW2 + H * H, kWh = kB2 + H, kBh = kWh + HI * 4;
  return PpoOffsets{HI, kB1, kW2, kB2, kWh, kBh, kBh + 4};
}
__host__ __device__ constexpr int ppo_buf_rows(int H) { return H > kPpoK ? H : kPpoK; }
__host__ __device__ constexpr size_t ppo_lds_bytes(int H) {
  return ((size_t)ppo_offsets(H).kNet + (size_t)2 * ppo_buf_rows(H) * kPpoPitch + (size_t)4 * kPpoPitch) * sizeof(float);
}
__host__ __device__ constexpr int ppo_slab_floats(int H) { return ppo_offsets(H).kNet + kPpoStatFloats; }

// the shape of a packed network, as the kernels read it
struct PpoShape {
  int n_in, n_out, n_hidden, w0, w1, act;
  int weight_floats;  // every W and b: the shift | scale | clip section starts here
  int set_floats;
};

// slab / LDS index of packed parameter e < weight_floats of `s` at padded width H (H == 0 iff n_hidden == 0)
__host__ __device__ inline int ppo_slab_index(int H, const PpoShape& s, int e) {
  const PpoOffsets o = ppo_offsets(H);
  if (s.n_hidden == 0) {  // the head reads the inputs
    const int nw = s.n_out * s.n_in;
    return e < nw ? o.kWh + 4 * (e % s.n_in) + e / s.n_in : o.kBh + (e - nw);
  }
  int nw = s.w0 * s.n_in;
  if (e < nw) return (e / s.n_in) * kPpoK + e % s.n_in;
  e -= nw;
  if (e < s.w0) return o.kB1 + e;
  e -= s.w0;
  int top = s.w0;
  if (s.n_hidden > 1) {
    nw = s.w1 * s.w0;
    if (e < nw) return o.kW2 + (e / s.w0) * H + e % s.w0;
    e -= nw;
    if (e < s.w1) return o.kB2 + e;
    e -= s.w1;
    top = s.w1;
  }
  nw = s.n_out * top;
  return e < nw ? o.kWh + 4 * (e % top) + e / top : o.kBh + (e - nw);
}

struct PpoNetArgs {
  carl_ppo_batch_t b;   // row_pitch resolved (never 0)
  PpoShape shape;
  int kind;             // kPpoCategorical / kPpoGaussian (the actor) / kPpoValue (the critic)
  int n_ctx;
  int ctx_rows[CARL_POLICY_MAX_IN];
  const float* params;  // the network's packed block
  const float* xform;   // shift [n_in] | scale [n_in] | clip of the ACTOR's packed block
  const float* log_std; // [1], Gaussian
  float* slab;          // [gridDim.x][ppo_slab_floats(H)]
  float* new_out;       // [n_samples] new_log_prob / new_value, nullable
  int n_tiles;
};

// d act(v) / dv from h = act(v)
__device__ __forceinline__ float ppo_act_grad(float h, int act) {
  if (act == CARL_POLICY_TANH) return __fmaf_rn(-h, h, 1.0f);
  if (act == CARL_POLICY_RELU) return h > 0.0f ? 1.0f : 0.0f;
  return 1.0f;
}

// row `row` of a tile buffer <- v for this thread's sample
__device__ __forceinline__ void ppo_put(float* buf, int row, float v) { buf[row * kPpoPitch + threadIdx.x] = v; }

// acc[r][c] += sum_s da[ri0 + r][s] * hb[cj0 + c][s] over the tile, s in index order (see the header comment)
template <int R, int Cn>
__device__ __forceinline__ void ppo_accumulate(const float* da, int ri0, const float* hb, int cj0, float (&acc)[R][Cn]) {
  float tile[R][Cn];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < Cn; ++c) tile[r][c] = 0.0f;
#pragma unroll 1
  for (int sb = 0; sb < kPpoTile; sb += 16) {
    float blk[R][Cn];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int c = 0; c < Cn; ++c) blk[r][c] = 0.0f;
#pragma unroll
    for (int s0 = 0; s0 < 16; s0 += 4) {
      pvf4 d[R], h[Cn];
#pragma unroll
      for (int r = 0; r < R; ++r) d[r] = bcast4(da + (ri0 + r) * kPpoPitch + sb + s0);
#pragma unroll
      for (int c = 0; c < Cn; ++c) h[c] = bcast4(hb + (cj0 + c) * kPpoPitch + sb + s0);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < Cn; ++c) {
          float a = blk[r][c];
          a = __fmaf_rn(d[r].x, h[c].x, a);
          a = __fmaf_rn(d[r].y, h[c].y, a);
          a = __fmaf_rn(d[r].z, h[c].z, a);
          a = __fmaf_rn(d[r].w, h[c].w, a);
          blk[r][c] = a;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int c = 0; c < Cn; ++c) tile[r][c] += blk[r][c];
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < Cn; ++c) acc[r][c] += tile[r][c];
}

// acc += sum_s da[row][s] over the tile, in the same order (a bias gradient)
__device__ __forceinline__ void ppo_accumulate_row(const float* da, int row, float& acc) {
  float tile = 0.0f;
#pragma unroll 1
  for (int sb = 0; sb < kPpoTile; sb += 16) {
    float blk = 0.0f;
#pragma unroll
    for (int s0 = 0; s0 < 16; s0 += 4) {
      const pvf4 d = bcast4(da + row * kPpoPitch + sb + s0);
      blk = ((blk + d.x) + d.y) + d.z + d.w;
    }
    tile += blk;
  }
  acc += tile;
}

// sum of v over the workgroup in a fixed order (float64), valid in thread 0; `red`: kPpoThreads doubles of LDS
__device__ __forceinline__ double ppo_block_sum(double* red, double v) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = kPpoThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

struct PpoReduceArgs {
  PpoShape actor, critic;
  int h_actor, h_critic;  // padded widths
  int n_workgroups;
  int gaussian;
  double inv_m;           // 1 / n_samples
  float n_samples;
  const float* slab_actor;   // [n_workgroups][the actor's slab floats at h_actor]
  const float* slab_critic;  // [n_workgroups][ppo_slab_floats(h_critic)]
  float* grad_actor;
  float* grad_critic;
  float* grad_log_std;
  float* stats;
};

// sum over the workgroups' slabs of entry `i`, in workgroup order, float64
__device__ __forceinline__ double ppo_slab_sum(const float* slab, int slab_floats, int n_workgroups, int i) {
  double s = 0.0;
  for (int g = 0; g < n_workgroups; ++g) s += (double)slab[(size_t)g * slab_floats + i];
  return s;
}

constexpr int kTraceThreads = 64;  // lanes per workgroup of the trace walk (ppo_kernels.hip.h: context_trace_kernel)

}  // namespace carl
