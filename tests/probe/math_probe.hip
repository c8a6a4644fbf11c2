// math_probe.hip -- one trivial kernel per device math primitive, for tests/test_gpu_math_primitives.py.
//
// The product's kernels reach these functions only inlined into a transition, at the arguments a policy visits.  Here each
// is evaluated on its own: inputs from arrays, the call, plain stores.  This unit is a TEST library (libcarl_math_probe.so,
// carl_amd/build.py: build_probe); it is not part of libcarl_amd.so and the product's sources do not change for it.
//
// ABI: every entry point takes device pointers, the element count n, the workgroup size `block` and a stream; it returns
// the hipError_t of the launch and never synchronises.  Thread i handles element i; threads past n do nothing (after the
// table kernels' stage + barrier, which every thread of a workgroup takes).
#include <hip/hip_runtime.h>

#include "brax_kernels.hip.h"
#include "classic_control.hip.h"

namespace probe {
using namespace carl;
using namespace carl::brax;

__device__ __forceinline__ int gid() { return blockIdx.x * blockDim.x + threadIdx.x; }

// ---- float -> (sin, cos)
__global__ void k_sincos_fast_f32(const float* x, float* s, float* c, int n) {
  const int i = gid();
  if (i < n) sincos_fast(x[i], s[i], c[i]);
}
__global__ void k_sincos_fast_pk(const float* x, float* s, float* c, int n) {
  const int i = gid();
  if (i < n) sincos_fast_pk(x[i], s[i], c[i]);
}
__global__ void k_sincos_fast_smallarg(const float* x, float* s, float* c, int n) {
  const int i = gid();
  if (i < n) sincos_fast_smallarg(x[i], s[i], c[i]);
}
// ---- double -> (sin, cos)
template <bool FALLBACK>
__global__ void k_sincos_fast_f64(const double* x, double* s, double* c, int n) {
  const int i = gid();
  if (i < n) sincos_fast<FALLBACK>(x[i], s[i], c[i]);
}
// ---- (double, double) -> (sin a, cos a, sin b, cos b)
__global__ void k_sincos2_fast(const double* xa, const double* xb, double* sa, double* ca, double* sb, double* cb, int n) {
  const int i = gid();
  if (i < n) sincos2_fast(xa[i], xb[i], sa[i], ca[i], sb[i], cb[i]);
}
__global__ void k_tab_sincos2(const double* xa, const double* xb, double* sa, double* ca, double* sb, double* cb, int n) {
  SinCosTab::stage();
  __syncthreads();
  const int i = gid();
  if (i < n) SinCosTab::sincos2(xa[i], xb[i], sa[i], ca[i], sb[i], cb[i]);
}
__global__ void k_tab_lookup_finish(const double* xa, const double* xb, double* sa, double* ca, double* sb, double* cb,
                                    int n) {
  SinCosTab::stage();
  __syncthreads();
  const int i = gid();
  if (i < n) {
    const SinCosTab::Pending q = SinCosTab::lookup2(xa[i], xb[i]);
    SinCosTab::finish2(q, sa[i], ca[i], sb[i], cb[i]);
  }
}
// what lookup2 hands to finish2: the table entries it read and the reduced arguments (out: n x 6 doubles)
__global__ void k_tab_lookup2(const double* xa, const double* xb, double* out, int n) {
  SinCosTab::stage();
  __syncthreads();
  const int i = gid();
  if (i < n) {
    const SinCosTab::Pending q = SinCosTab::lookup2(xa[i], xb[i]);
    double* o = out + 6 * (size_t)i;
    o[0] = q.ea.x; o[1] = q.ea.y; o[2] = q.eb.x; o[3] = q.eb.y; o[4] = q.ra; o[5] = q.rb;
  }
}
// the staged table itself: workgroup b writes its LDS copy to out[b][CARL_SINCOS_TAB_N][2]
__global__ void k_tab_stage(double* out) {
  SinCosTab::stage();
  __syncthreads();
  const SinCosTab::vd2* t = SinCosTab::lds();
  double* o = out + (size_t)blockIdx.x * 2 * CARL_SINCOS_TAB_N;
  for (int i = threadIdx.x; i < CARL_SINCOS_TAB_N; i += blockDim.x) {
    o[2 * i] = t[i].x;
    o[2 * i + 1] = t[i].y;
  }
}

// ---- unary / binary scalar functions
#define PROBE_UNARY(NAME, T, EXPR)                         \
  __global__ void k_##NAME(const T* x, T* y, int n) {     \
    const int i = gid();                                   \
    if (i < n) { const T a = x[i]; y[i] = (EXPR); }        \
  }
#define PROBE_BINARY(NAME, T, EXPR)                                    \
  __global__ void k_##NAME(const T* x0, const T* x1, T* y, int n) {   \
    const int i = gid();                                               \
    if (i < n) { const T a = x0[i], b = x1[i]; y[i] = (EXPR); }        \
  }
PROBE_UNARY(rcp_fast, double, rcp_fast(a))
PROBE_UNARY(rcp_fast1, double, rcp_fast1(a))
PROBE_UNARY(cos_fast, float, cos_fast(a))
PROBE_UNARY(cos_twice_fast, float, cos_twice_fast(a))
PROBE_UNARY(sqrt01_f64, double, sqrt01_f64(a))
PROBE_UNARY(asin_f64, double, asin_f64(a))
PROBE_UNARY(asin_r_f64, double, asin_r(a))
PROBE_UNARY(asin_r_f32, float, asin_r(a))
PROBE_BINARY(atan2_fast, float, atan2_fast(a, b))
PROBE_BINARY(div_fast, float, div_fast(a, b))
PROBE_BINARY(atan2_f64, double, atan2_f64<false>(a, b))
PROBE_BINARY(atan2_f64_xpos, double, atan2_f64<true>(a, b))
PROBE_BINARY(atan2_r_f64, double, atan2_r<false>(a, b))
PROBE_BINARY(atan2_r_f64_xpos, double, atan2_r<true>(a, b))
PROBE_BINARY(atan2_r_f32, float, atan2_r<false>(a, b))

// (k, angle) -> quaternion w x y z (out: n x 4 floats)
__global__ void k_qaxis(const int* k, const float* angle, float* out, int n) {
  const int i = gid();
  if (i < n) {
    const qt q = qaxis(k[i], angle[i]);
    float* o = out + 4 * (size_t)i;
    o[0] = q.w; o[1] = q.x; o[2] = q.y; o[3] = q.z;
  }
}

template <class K, class... A>
hipError_t launch(K kernel, int n, int block, void* stream, A... args) {
  if (n <= 0 || block <= 0 || block > 1024) return hipErrorInvalidValue;
  const int grid = (n + block - 1) / block;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, args..., n);
  return hipGetLastError();
}
}  // namespace probe

using namespace probe;
#define ENTRY_SC(NAME, T, KERNEL)                                                                      \
  extern "C" int probe_##NAME(const T* x, T* s, T* c, int n, int block, void* stream) {                \
    return (int)launch(KERNEL, n, block, stream, x, s, c);                                             \
  }
#define ENTRY_SC2(NAME, KERNEL)                                                                        \
  extern "C" int probe_##NAME(const double* xa, const double* xb, double* sa, double* ca, double* sb,  \
                              double* cb, int n, int block, void* stream) {                            \
    return (int)launch(KERNEL, n, block, stream, xa, xb, sa, ca, sb, cb);                              \
  }
#define ENTRY_UNARY(NAME, T)                                                                           \
  extern "C" int probe_##NAME(const T* x, T* y, int n, int block, void* stream) {                      \
    return (int)launch(k_##NAME, n, block, stream, x, y);                                              \
  }
#define ENTRY_BINARY(NAME, T)                                                                          \
  extern "C" int probe_##NAME(const T* x0, const T* x1, T* y, int n, int block, void* stream) {        \
    return (int)launch(k_##NAME, n, block, stream, x0, x1, y);                                         \
  }

ENTRY_SC(sincos_fast_f32, float, k_sincos_fast_f32)
ENTRY_SC(sincos_fast_pk, float, k_sincos_fast_pk)
ENTRY_SC(sincos_fast_smallarg, float, k_sincos_fast_smallarg)
ENTRY_SC(sincos_fast_f64, double, k_sincos_fast_f64<true>)
ENTRY_SC(sincos_fast_f64_nofallback, double, k_sincos_fast_f64<false>)
ENTRY_SC2(sincos2_fast, k_sincos2_fast)
ENTRY_SC2(tab_sincos2, k_tab_sincos2)
ENTRY_SC2(tab_lookup_finish, k_tab_lookup_finish)
ENTRY_UNARY(rcp_fast, double)
ENTRY_UNARY(rcp_fast1, double)
ENTRY_UNARY(cos_fast, float)
ENTRY_UNARY(cos_twice_fast, float)
ENTRY_UNARY(sqrt01_f64, double)
ENTRY_UNARY(asin_f64, double)
ENTRY_UNARY(asin_r_f64, double)
ENTRY_UNARY(asin_r_f32, float)
ENTRY_BINARY(atan2_fast, float)
ENTRY_BINARY(div_fast, float)
ENTRY_BINARY(atan2_f64, double)
ENTRY_BINARY(atan2_f64_xpos, double)
ENTRY_BINARY(atan2_r_f64, double)
ENTRY_BINARY(atan2_r_f64_xpos, double)
ENTRY_BINARY(atan2_r_f32, float)

extern "C" int probe_tab_lookup2(const double* xa, const double* xb, double* out, int n, int block, void* stream) {
  return (int)launch(k_tab_lookup2, n, block, stream, xa, xb, out);
}
extern "C" int probe_qaxis(const int* k, const float* angle, float* out, int n, int block, void* stream) {
  return (int)launch(k_qaxis, n, block, stream, k, angle, out);
}
// out: n_blocks x CARL_SINCOS_TAB_N x 2 doubles
extern "C" int probe_tab_stage(double* out, int n_blocks, int block, void* stream) {
  if (n_blocks <= 0 || block <= 0 || block > 1024) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tab_stage, dim3(n_blocks), dim3(block), 0, (hipStream_t)stream, out);
  return (int)hipGetLastError();
}
extern "C" int probe_tab_entries(void) { return CARL_SINCOS_TAB_N; }
