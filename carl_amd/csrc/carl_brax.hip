// carl_brax.hip -- C-ABI entry points of the Brax-locomotion families (include/carl_amd.h) and
// their kernel dispatch.  A translation unit of its own because it is compiled with
// -fno-slp-vectorize: the SLP vectoriser packs the per-lane 3-vector algebra into v_pk_*_f32
// pairs and then spends as many v_mov as it saved to build the register pairs; the kernel is
// bound by instruction issue, and without packing it is 9-22 % faster (profiles/r01g).  (Round 4: the classic-control
// unit is built with the same flag -- carl_amd/build.py; its one useful packing is written by hand.)
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/carl_amd.h"
#include "brax_kernels.hip.h"
#include "brax_launch.hpp"
#include "host_common.hpp"

namespace {

using carl_host::check_launch;
using carl_host::fail;
using carl_host::brax::brax_class;
using carl_host::brax::brax_is_planar;
using carl_host::brax::BraxClass;
using carl_host::brax::BraxShape;
using carl_host::brax::same_class;
using carl_host::brax::validate_brax;
using carl_host::brax::validate_brax_io;

// (the checks of a batch and its model, the kernel class of a model -- lean / multi-hinge / general / planar -- and the
// launch-shape rule live in brax_launch.hpp, shared with the closed-loop rollout's unit)

// Every instantiated brax_kernel<MODE, MULTI, K, TASK, PLANAR, F32>: (class, K) -> its reset and step kernels.
using brax_kern_t = void (*)(carl_batch_t, const carl_brax_sys_t*, carl::brax::Prepared, carl_step_io_t, const uint8_t*,
                             float*, int);
struct BraxKernel {
  BraxClass c;
  int k;
  brax_kern_t reset, step;
};
#define CARL_BRAX(MULTI, K, TASK) \
  {{MULTI, TASK, false, false}, K, carl::brax::brax_kernel<0, MULTI, K, TASK>, carl::brax::brax_kernel<1, MULTI, K, TASK>}
#define CARL_BRAX_STEP(MULTI, K, PLANAR, F32) \
  {{MULTI, false, PLANAR, F32}, K, nullptr, carl::brax::brax_kernel<1, MULTI, K, false, PLANAR, F32>}
const BraxKernel kBraxKernels[] = {
    // lean (a free root and single hinges: Ant)
    CARL_BRAX(false, 4, false), CARL_BRAX(false, 7, false), CARL_BRAX(false, 8, false), CARL_BRAX(false, 9, false),
    CARL_BRAX(false, 16, false),
    // multi-hinge
    CARL_BRAX(true, 2, false), CARL_BRAX(true, 11, false), CARL_BRAX(true, 16, false),
    // general: reach / push task models (reacher: 3 links, pusher: 8) and anisotropic inertia
    CARL_BRAX(true, 4, true), CARL_BRAX(true, 8, true), CARL_BRAX(true, 16, true),
    // planar
    CARL_BRAX_STEP(false, 4, true, false), CARL_BRAX_STEP(false, 7, true, false), CARL_BRAX_STEP(false, 8, true, false),
    CARL_BRAX_STEP(false, 9, true, false), CARL_BRAX_STEP(false, 16, true, false),
    // CARL_FLAG_BRAX_FP32 (opt-in): the same kernels with the substeps' pose algebra in float32
    CARL_BRAX_STEP(false, 4, false, true), CARL_BRAX_STEP(false, 7, false, true), CARL_BRAX_STEP(false, 8, false, true),
    CARL_BRAX_STEP(false, 9, false, true), CARL_BRAX_STEP(false, 16, false, true),
    CARL_BRAX_STEP(true, 2, false, true), CARL_BRAX_STEP(true, 11, false, true), CARL_BRAX_STEP(true, 16, false, true),
    CARL_BRAX_STEP(false, 4, true, true), CARL_BRAX_STEP(false, 7, true, true), CARL_BRAX_STEP(false, 8, true, true),
    CARL_BRAX_STEP(false, 9, true, true), CARL_BRAX_STEP(false, 16, true, true),
};
#undef CARL_BRAX
#undef CARL_BRAX_STEP

// the kernel class and the shape of a reset (step false) or step / rollout launch: what launch_brax launches and
// carl_brax_launch_shape reports
int class_and_shape(const carl_batch_t* b, const carl_brax_sys_t* sh, bool step, int n_steps, const char* who, BraxClass* c,
                    BraxShape* shape) {
  *c = brax_class(sh, b->flags, step);
  if (c->f32 && c->task)
    return fail(CARL_ERR_UNSUPPORTED, "%s: CARL_FLAG_BRAX_FP32 is not built for the reach / push task models or anisotropic inertia", who);
  return carl_host::brax::brax_launch_shape(kBraxKernels, b, sh, *c, step, n_steps, false, who, shape);
}

template <int MODE>
int launch_brax(const carl_batch_t* b, const carl_brax_sys_t* sd, const carl_brax_sys_t* sh,
                       const carl_step_io_t* io, const uint8_t* mask, float* reset_obs, int n_steps, hipStream_t st,
                       const char* who) {
  if (b->n_lanes == 0 || (MODE == 1 && n_steps == 0)) return 0;
  BraxClass c;
  BraxShape shape;
  if (int e = class_and_shape(b, sh, MODE == 1, n_steps, who, &c, &shape)) return e;
  const int K = shape.K, W = shape.W, grid = shape.grid;
  const size_t sh_bytes = shape.lds_bytes;
  brax_kern_t kern = nullptr;
  for (const BraxKernel& e : kBraxKernels)
    if (same_class(e.c, c) && e.k == K) kern = MODE == 0 ? e.reset : e.step;
  if (kern == nullptr) return fail(CARL_ERR_UNSUPPORTED, "%s: no kernel for %d lanes per env", who, K);
  if (sh_bytes > 48 * 1024) {
    if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(kern), sh_bytes, who)) return e;
  }
  carl_step_io_t io_v{};
  if (io != nullptr) io_v = *io;
  const carl::brax::Prepared prep = carl_host::brax::make_prepared(sh);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(carl::brax::kLanes * W), sh_bytes, st, *b, sd, prep, io_v, mask, reset_obs,
                     n_steps);
  return check_launch(who);
}

}  // namespace

extern "C" {

int carl_brax_reset(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                    const uint8_t* mask, float* obs, void* stream) {
  if (int e = validate_brax(batch, sys_dev, sys_host, "carl_brax_reset")) return e;
  return launch_brax<0>(batch, sys_dev, sys_host, nullptr, mask, obs, 0, (hipStream_t)stream, "carl_brax_reset");
}

int carl_brax_step(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                   const carl_step_io_t* io, void* stream) {
  if (int e = validate_brax(batch, sys_dev, sys_host, "carl_brax_step")) return e;
  if (int e = validate_brax_io(io, "carl_brax_step")) return e;
  return launch_brax<1>(batch, sys_dev, sys_host, io, nullptr, nullptr, 1, (hipStream_t)stream, "carl_brax_step");
}

int carl_brax_rollout(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                      const carl_step_io_t* io, int32_t n_steps, void* stream) {
  if (int e = validate_brax(batch, sys_dev, sys_host, "carl_brax_rollout")) return e;
  if (int e = validate_brax_io(io, "carl_brax_rollout")) return e;
  if (n_steps < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "carl_brax_rollout: n_steps %d < 0", n_steps);
  return launch_brax<1>(batch, sys_dev, sys_host, io, nullptr, nullptr, n_steps, (hipStream_t)stream,
                        "carl_brax_rollout");
}

int carl_brax_fragment_plan(int32_t n_groups, int32_t n_workgroups, int32_t waves_per_workgroup, int32_t n_steps,
                            int32_t workgroup, int32_t wave, int32_t* out, int32_t cap) {
  if (n_groups < 1 || n_workgroups < 1 || waves_per_workgroup < 1 || n_steps < 1 || workgroup < 0 ||
      workgroup >= n_workgroups || wave < 0 || wave >= waves_per_workgroup || (cap > 0 && out == nullptr)) {
    fail(CARL_ERR_INVALID_ARGUMENT, "carl_brax_fragment_plan: argument out of range");
    return -1;
  }
  const carl::brax::WgShare sh = carl::brax::wg_share(n_groups, n_workgroups, workgroup);
  const carl::brax::Piece p = carl::brax::make_piece(sh.G, n_steps, waves_per_workgroup, wave);
  for (int fi = 0; fi < p.n_frag && fi < cap; ++fi) {
    const carl::brax::Fragment f = carl::brax::fragment_of(p, n_steps, fi);
    int32_t* o = out + 5 * fi;
    o[0] = sh.g_lo + f.grp; o[1] = f.t_lo; o[2] = f.t_hi; o[3] = f.wait_head ? 1 : 0; o[4] = f.signal_head ? 1 : 0;
  }
  return p.n_frag;
}

#ifdef CARL_BRAX_PROFILE
// measurement build only (not declared in include/carl_amd.h): the region clocks of brax_kernels.hip.h, summed over every
// wavefront since the last reset; out[kProfRegions] = wavefronts
int carl_brax_profile_read(unsigned long long* out, int reset) {
  unsigned long long zero[carl::brax::kProfRegions + 1] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(carl::brax::g_brax_prof), sizeof(zero)) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(carl::brax::g_brax_prof), zero, sizeof(zero)) != hipSuccess) return -1;
  return carl::brax::kProfRegions;
}
#endif

int carl_brax_launch_shape(const carl_batch_t* batch, const carl_brax_sys_t* sys_host, int32_t step, int32_t n_steps,
                           carl_brax_launch_shape_t* out) {
  const char* who = "carl_brax_launch_shape";
  if (batch == nullptr || sys_host == nullptr || out == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  if (batch->n_lanes < 1 || (step != 0 && n_steps < 1) || sys_host->n_links < 1 || sys_host->n_links > CARL_BRAX_MAX_LINKS)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d / n_links %d out of range", who, batch->n_lanes, n_steps,
                sys_host->n_links);
  BraxClass c;
  BraxShape shape;
  if (int e = class_and_shape(batch, sys_host, step != 0, step != 0 ? n_steps : 0, who, &c, &shape)) return e;
  *out = carl_brax_launch_shape_t{shape.grid, shape.W, shape.K, 0, (int64_t)shape.lds_bytes};
  return 0;
}

int carl_brax_model_is_planar(const carl_brax_sys_t* sys_host) {
  if (sys_host == nullptr) {
    fail(CARL_ERR_INVALID_ARGUMENT, "carl_brax_model_is_planar: NULL argument");
    return 0;
  }
  return brax_is_planar(sys_host) ? 1 : 0;
}

int carl_brax_lane_widths(const carl_brax_sys_t* sys_host, uint32_t batch_flags, int32_t* widths_out, int32_t cap) {
  if (sys_host == nullptr || widths_out == nullptr || cap < 1) {
    fail(CARL_ERR_INVALID_ARGUMENT, "carl_brax_lane_widths: NULL argument");
    return 0;
  }
  // the kernels a STEP / ROLLOUT launch of such a batch takes (launch_brax<1>): a planar model stepped by the general
  // substep (CARL_FLAG_BRAX_GENERIC) runs the multi-hinge kernels, whose widths differ from the planar ones
  const BraxClass c = brax_class(sys_host, batch_flags, true);
  int n = 0;
  using carl_host::brax::brax_width_from;
  for (int w = brax_width_from(kBraxKernels, c, sys_host->n_links); w != 0 && n < cap; w = brax_width_from(kBraxKernels, c, w + 1))
    widths_out[n++] = w;  // one lane per link or wider
  return n;
}

}  // extern "C"
