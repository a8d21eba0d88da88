// mvm_internal.h — host helpers shared by the library's translation units (not
// part of the public C ABI).  Errors are recorded per thread for
// mvm_last_error_string().
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "mvmatch.h"

// f(std::true_type) or f(std::false_type): a launch written once for both
// values of a kernel's bool template parameter
template <typename F>
void dispatch_bool(bool b, F &&f) {
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}
// f(std::integral_constant<int, V>) for the V among Vs... that v equals (none:
// f is not called): the same for an int template parameter
template <int... Vs, typename F>
void dispatch_int(int v, F &&f) {
    (void)((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

int mvm_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void mvm_set_error(const char *msg);
void mvm_clear_error();
int mvm_check_launch(const char *what);
// MVM_OK, or MVM_ERR_INVALID_ARGUMENT with "null pointer: <name>" recorded for
// the first NULL of {pointer, name}, ...
struct mvm_named_ptr {
    const void *p;
    const char *name;
};
int mvm_require_ptrs(std::initializer_list<mvm_named_ptr> args);
// *in (NULL = defaults) -> out, every field present; MVM_OK or an error code
int mvm_resolve_options(const mvm_options *in, mvm_options &out);
// dynamic LDS above 64 KiB needs the kernel's opt-in; MVM_OK or MVM_ERR_HIP
int mvm_raise_dynamic_lds(const void *kernel, size_t bytes);
// an option bounding a kernel class: 0 = dflt, negative = off (0), at most cap
int mvm_resolve_limit(int32_t opt, int dflt, int cap);
// workgroups the device holds at once (CUs x occupancy), 0 if a query fails
int64_t mvm_coresident_blocks(const void *kernel, int threads, size_t lds);
// The LSAP plans' loop: n + 1 offsets of the workspace regions and the output
// pairs; need(nr, nc, tr, elem) = region of a non-empty nr <= nc problem (tr:
// given tall).  The workspace total, or -1 with "<who>: ..." recorded.
int64_t mvm_lsap_plan_offsets(const char *who, int32_t n, const int64_t *rows, const int64_t *cols,
                              size_t elem, int64_t (*need)(int64_t nr, int64_t nc, bool tr, size_t elem),
                              int64_t *ws_offs, int64_t *out_offs);
