// The query entries of the C ABI, generated from the entry table (csrc/abi_table.h): ABI version, device count, struct sizes and
// the scratch bytes of every stream entry.  A row that names another struct than the header's prototype does not compile.
#include <string.h>
#include <type_traits>
#include "common.h"
#include "../../include/wavjepa_hip.h"
#ifdef WJ_LAB
#include "../../include/wavjepa_hip_lab.h"
#endif
#include "abi_table.h"

#define WJ_ROW_CHECK(entry, ARGS, ...) \
    static_assert(std::is_same_v<decltype(&entry), int (*)(const ARGS*, void*)>, #entry " does not take " #ARGS " in the header");
WJ_STREAM_ENTRIES(WJ_ROW_CHECK, WJ_ROW_CHECK)

#define WJ_NO_DECL(entry, ARGS)
#define WJ_RULE_DECL(entry, ARGS, rule) int64_t rule(const ARGS*);
WJ_STREAM_ENTRIES(WJ_NO_DECL, WJ_RULE_DECL)

extern "C" int wj_abi_version(void) { return WJ_ABI_VERSION; }
extern "C" int wj_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int wj_struct_size(const char* name) {
    if (!name) return -1;
#define WJ_SZ(T) if (!strcmp(name, #T)) return (int)sizeof(T);
#define WJ_ROW_SZ(entry, ARGS, ...) WJ_SZ(ARGS)
    WJ_STREAM_ENTRIES(WJ_ROW_SZ, WJ_ROW_SZ)
    WJ_OTHER_STRUCTS(WJ_SZ)
    return -1;
}

extern "C" int64_t wj_workspace_bytes(const char* fn, const void* args) {
    if (!fn || !args) return -1;
#define WJ_ROW_NONE(entry, ARGS) if (!strcmp(fn, #entry)) return 0;
#define WJ_ROW_RULE(entry, ARGS, rule) if (!strcmp(fn, #entry)) return rule((const ARGS*)args);
    WJ_STREAM_ENTRIES(WJ_ROW_NONE, WJ_ROW_RULE)
    return -1;
}
