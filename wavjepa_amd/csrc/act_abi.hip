// The query entries of libwavjepa_hip_act.so, generated from its row of the entry table (csrc/abi_table.h) as csrc/abi.hip generates
// libwavjepa_hip.so's: struct sizes and scratch bytes; a row that names another struct than the header's prototype does not compile.
#include <string.h>
#include <type_traits>
#include "common.h"
#include "../../include/wavjepa_hip_act.h"
#include "abi_table.h"

#define WJ_ACT_EXPORT __attribute__((visibility("default")))

#define WJ_ROW_CHECK(entry, ARGS, ...) \
    static_assert(std::is_same_v<decltype(&entry), int (*)(const ARGS*, void*)>, #entry " does not take " #ARGS " in the header");
WJ_ACT_ENTRIES(WJ_ROW_CHECK, WJ_ROW_CHECK)

#define WJ_NO_DECL(entry, ARGS)
#define WJ_RULE_DECL(entry, ARGS, rule) int64_t rule(const ARGS*);
WJ_ACT_ENTRIES(WJ_NO_DECL, WJ_RULE_DECL)

extern "C" WJ_ACT_EXPORT int wj_act_struct_size(const char* name) {
    if (!name) return -1;
#define WJ_SZ(T) if (!strcmp(name, #T)) return (int)sizeof(T);
#define WJ_ROW_SZ(entry, ARGS, ...) WJ_SZ(ARGS)
    WJ_ACT_ENTRIES(WJ_ROW_SZ, WJ_ROW_SZ)
    return -1;
}

extern "C" WJ_ACT_EXPORT int64_t wj_act_workspace_bytes(const char* fn, const void* args) {
    if (!fn || !args) return -1;
#define WJ_ROW_NONE(entry, ARGS) if (!strcmp(fn, #entry)) return 0;
#define WJ_ROW_RULE(entry, ARGS, rule) if (!strcmp(fn, #entry)) return rule((const ARGS*)args);
    WJ_ACT_ENTRIES(WJ_ROW_NONE, WJ_ROW_RULE)
    return -1;
}
