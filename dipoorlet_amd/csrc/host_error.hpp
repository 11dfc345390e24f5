// The library's error text (dpl_last_error) and the host-only way to set it.  No HIP in here: common.hpp includes this for
// every kernel translation unit, host_plan.hpp for the host planning code, which a plain C++ compiler must be able to build.
#pragma once
#include <stdio.h>

namespace dpl {
inline thread_local char g_err[512] = "";  // one per thread for the whole library (shared by every translation unit)
}

namespace {

using dpl::g_err;

int fail_msg(const char* what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return -2;
}

}  // namespace
