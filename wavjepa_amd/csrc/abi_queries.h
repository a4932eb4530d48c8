// The query entries of every library, generated from its rows of the entry table (csrc/abi_table.h): one generator, used once per library
// (csrc/abi.hip, dropout.hip, gemm.hip under WJ_ACT_LIB, monitor.hip, optim.hip).  Include the library's header(s) first.
//   WJ_ABI_QUERIES(ENTRIES, OTHER_STRUCTS, struct_size, workspace_bytes)
// checks every row against the header's prototype (a row that names another struct does not compile), declares the rules, and defines
//   int struct_size(const char* name)                           sizeof of the row's / the list's struct; -1 for NULL or an unknown name
//   int64_t workspace_bytes(const char* fn, const void* args)   0 for an E row, the rule's answer for a W row; -1 for NULL or an unknown name
#pragma once
#include <string.h>
#include <type_traits>
#include "common.h"
#include "abi_table.h"

#define WJ_ROW_CHECK(entry, ARGS, ...) \
    static_assert(std::is_same_v<decltype(&entry), int (*)(const ARGS*, void*)>, #entry " does not take " #ARGS " in the header");
#define WJ_NO_DECL(entry, ARGS)
#define WJ_RULE_DECL(entry, ARGS, rule) int64_t rule(const ARGS*);
#define WJ_SZ(T) if (!strcmp(name, #T)) return (int)sizeof(T);
#define WJ_ROW_SZ(entry, ARGS, ...) WJ_SZ(ARGS)
#define WJ_ROW_NONE(entry, ARGS) if (!strcmp(fn, #entry)) return 0;
#define WJ_ROW_RULE(entry, ARGS, rule) if (!strcmp(fn, #entry)) return rule((const ARGS*)args);

#define WJ_ABI_QUERIES(ENTRIES, OTHER_STRUCTS, struct_size, workspace_bytes)                    \
    ENTRIES(WJ_ROW_CHECK, WJ_ROW_CHECK)                                                         \
    ENTRIES(WJ_NO_DECL, WJ_RULE_DECL)                                                           \
    extern "C" WJ_EXPORT int struct_size(const char* name) {                                    \
        if (!name) return -1;                                                                   \
        ENTRIES(WJ_ROW_SZ, WJ_ROW_SZ)                                                           \
        OTHER_STRUCTS(WJ_SZ)                                                                    \
        return -1;                                                                              \
    }                                                                                           \
    extern "C" WJ_EXPORT int64_t workspace_bytes(const char* fn, const void* args) {            \
        if (!fn || !args) return -1;                                                            \
        ENTRIES(WJ_ROW_NONE, WJ_ROW_RULE)                                                       \
        return -1;                                                                              \
    }
