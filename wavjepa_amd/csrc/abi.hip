// The query entries of the C ABI: ABI version, device count and, generated from the entry table (csrc/abi_queries.h), struct sizes and
// the scratch bytes of every stream entry.
#include "../../include/wavjepa_hip.h"
#ifdef WJ_LAB
#include "../../include/wavjepa_hip_lab.h"
#endif
#include "abi_queries.h"

extern "C" int wj_abi_version(void) { return WJ_ABI_VERSION; }
extern "C" int wj_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

WJ_ABI_QUERIES(WJ_STREAM_ENTRIES, WJ_OTHER_STRUCTS, wj_struct_size, wj_workspace_bytes)
