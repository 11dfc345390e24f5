// The part of the C ABI that is not about a kernel: version, error text, device info, streams.
#include "common.hpp"

extern "C" {

int dpl_abi_version(void) { return DPL_ABI_VERSION; }
const char* dpl_last_error(void) { return g_err; }

int dpl_device_info(char* name, int name_cap, int* compute_units, uint64_t* hbm_bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail("hipGetDevice", e);
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return fail("hipGetDeviceProperties", e);
    if (name && name_cap > 0) snprintf(name, name_cap, "%s (%s)", p.name, p.gcnArchName);
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return fail_msg("current HIP device is not gfx950");
    return 0;
}

int dpl_stream_priority_range(int* least, int* greatest) {
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (e != hipSuccess) return fail("hipDeviceGetStreamPriorityRange", e);
    if (least) *least = lo;
    if (greatest) *greatest = hi;
    return 0;
}

int dpl_stream_create(int priority, dpl_stream_t* out) {
    if (!out) return fail_msg("dpl_stream_create: null out");
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);   // (lo: the numerically largest = least urgent)
    if (e != hipSuccess) return fail("hipDeviceGetStreamPriorityRange", e);
    if (priority > lo) priority = lo;
    if (priority < hi) priority = hi;
    hipStream_t s = nullptr;
    e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    if (e != hipSuccess) return fail("hipStreamCreateWithPriority", e);
    *out = (dpl_stream_t)s;
    return 0;
}

int dpl_stream_destroy(dpl_stream_t s) {
    if (!s) return 0;
    hipError_t e = hipStreamDestroy((hipStream_t)s);
    return e == hipSuccess ? 0 : fail("hipStreamDestroy", e);
}

}  // extern "C"
