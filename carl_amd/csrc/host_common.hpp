// host_common.hpp -- host-side rules shared by the translation units of libcarl_amd.so (defined in carl_amd.hip): error
// reporting, the batch checks of every classic-control entry point, the staged row layout
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/carl_amd.h"

namespace carl_host {
extern thread_local char g_err[512];
int fail(int code, const char* fmt, ...);  // formats into g_err, returns code
int check_launch(const char* what);        // hipGetLastError -> 0 / fail(...)
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel, size) instead of on every launch
// (it is a driver call: ~2 us of the ~10 us a launch costs the host)
int ensure_dynamic_lds(const void* kernel, size_t bytes, const char* who);

// a classic-control batch: family, sizes, selector, pointers, context observation features, finished-episode log
int validate_batch(const carl_batch_t* b, const char* who);
// whether the rows of `io` take the staged layout (carl_step_io_t::row_pitch); action_align_mask: the alignment the
// action array needs, minus one
bool staged_rows(const carl_batch_t* b, const carl_step_io_t* io, uintptr_t action_align_mask);
}  // namespace carl_host
