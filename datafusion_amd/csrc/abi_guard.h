// The error frame of the C ABI (no device in it: exec_internal.h brings it to
// the device-side entry points, agg_host.cpp includes it alone): an entry
// point's body throws Fail; the frame turns it into the dfmi_error and the
// returned code.
#pragma once
#include <cstdio>
#include <string>

#include "../../include/dfmi.h"

namespace dfmi {

struct Fail {
    int32_t code;
    std::string msg;
};

namespace xi {

inline void set_err(dfmi_error* err, int32_t code, const std::string& m) {
    if (!err) return;
    err->code = code;
    snprintf(err->message, sizeof err->message, "%s", m.c_str());
}

// `err` cleared, then body(); a Fail becomes `err` and its code, after
// on_fail() has released what the body left half done.
template <class F, class C>
inline int32_t guarded(dfmi_error* err, F&& body, C&& on_fail) {
    set_err(err, DFMI_OK, "");
    try {
        return body();
    } catch (const Fail& f) {
        on_fail();
        set_err(err, f.code, f.msg);
        return f.code;
    }
}
template <class F>
inline int32_t guarded(dfmi_error* err, F&& body) {
    return guarded(err, body, [] {});
}

// ... for the entry points that return a size, or -(code).
template <class F>
inline int64_t guarded_size(dfmi_error* err, F&& body) {
    set_err(err, DFMI_OK, "");
    try {
        return body();
    } catch (const Fail& f) {
        set_err(err, f.code, f.msg);
        return -(int64_t)f.code;
    }
}

}  // namespace xi
}  // namespace dfmi
