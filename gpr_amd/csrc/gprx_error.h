// gprx_error.h — the library's host error type (no device or runtime headers: the host-only
// units, pt_sched.cpp, include it alone; gprx_internal.h includes it for everything else).
#pragma once

#include <string>

#include "../../include/gprx.h"

namespace gprx {

struct Error {
    gprx_status st;
    std::string msg;
};

}  // namespace gprx

#define GPRX_REQUIRE(cond, status, msg)                                                            \
    do {                                                                                           \
        if (!(cond)) throw ::gprx::Error{status, msg};                                             \
    } while (0)
