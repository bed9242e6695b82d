// Error plumbing and misc entry points of the C ABI (include/arrow_amd.h).
#include "arx_common.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace arx {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) in %s", static_cast<int>(e), hipGetErrorString(e), what);
  (void)hipGetLastError();  // clear the sticky error
  return e == hipErrorOutOfMemory ? ARX_OUT_OF_MEMORY : ARX_DEVICE_ERROR;
}

// The knob / the counter of this name in the files' tables, or nullptr (with the error set).
static const KnobRow* find_knob(const char* name) {
  const KnobTable tables[] = {selection_knobs(), sort_knobs(), groupby_knobs(), groupby_lines_knobs(), parquet_knobs()};
  if (name != nullptr) {
    for (const KnobTable& t : tables) {
      for (size_t i = 0; i < t.n; ++i) {
        if (strcmp(name, t.rows[i].name) == 0) return &t.rows[i];
      }
    }
  }
  if (name == nullptr) set_error("option name is NULL");
  else set_error("unknown option '%s'", name);
  return nullptr;
}

static const CounterRow* find_counter(const char* name) {
  const CounterTable tables[] = {groupby_counters(), groupby_lines_counters(), sort_counters(), set_lookup_counters(),
                                 match_substring_counters(), if_else_counters(), temporal_counters(), string_slice_counters(),
                                 string_trim_counters(), string_compare_counters(), string_replace_counters(), string_join_counters(),
                                 unary_arith_counters(), case_when_counters(), element_wise_counters()};
  if (name != nullptr) {
    for (const CounterTable& t : tables) {
      for (size_t i = 0; i < t.n; ++i) {
        if (strcmp(name, t.rows[i].name) == 0) return &t.rows[i];
      }
    }
  }
  set_error("unknown counter '%s'", name == nullptr ? "(null)" : name);
  return nullptr;
}

}  // namespace arx

extern "C" {

const char* arx_last_error(void) { return arx::g_error; }

int arx_abi_version(void) { return ARX_ABI_VERSION; }

int arx_set_option(const char* name, int64_t value) {
  const arx::KnobRow* k = arx::find_knob(name);
  if (k == nullptr) return ARX_INVALID;
  const int64_t v = k->rule != nullptr ? k->rule(value) : std::max(k->lo, std::min(value, k->hi));
  if (k->k64 != nullptr) *k->k64 = v;
  else *k->k32 = static_cast<int>(v);
  return ARX_OK;
}

int arx_get_option(const char* name, int64_t* out_value) {
  const arx::KnobRow* k = arx::find_knob(name);
  if (k == nullptr) return ARX_INVALID;
  if (out_value == nullptr) {
    arx::set_error("out_value is NULL");
    return ARX_INVALID;
  }
  *out_value = k->k64 != nullptr ? int64_t(*k->k64) : int64_t(int(*k->k32));
  return ARX_OK;
}

int64_t arx_get_counter(const char* name) {
  const arx::CounterRow* c = arx::find_counter(name);
  return c != nullptr ? c->v->load() : -1;
}

int arx_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return arx::hip_fail(e, "hipGetDeviceCount");
  return n;
}

}  // extern "C"
