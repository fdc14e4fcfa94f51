// What belongs to libhipac_hip.so as a whole: the ABI version and the per-thread error text every entry point sets.
#include <stdarg.h>
#include <stdio.h>

#include "common.h"

namespace hipac {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

}  // namespace hipac

extern "C" {

int hipac_abi_version(void) { return HIPAC_ABI_VERSION; }
const char* hipac_last_error(void) { return hipac::g_err; }

}  // extern "C"
