// Marks an entry point of the host runtime library: flat C ABI, exported. The same marker as the
// kernel library's (csrc/common.h), so that one parser (ops/build.py api_signatures) derives the
// ctypes signatures of both libraries from the definitions that carry it. The parameter and
// return types of a marked function come from the table in ops/build.py.
#pragma once

#define FMLX_API extern "C" __attribute__((visibility("default")))
