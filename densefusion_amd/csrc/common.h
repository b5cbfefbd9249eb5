// Shared helpers for libdfusion_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdlib>
#include <cstdint>
#include <cstdio>

#include "../../include/dfusion.h"

namespace df {

constexpr int DF_MAX_CROP = 3200;      // largest crop side the network entry points take (LDS tables of psp_prior_sum, layers.hip)

int set_error(int code, const char *fmt, ...);   // records a thread-local message, returns code
int check_launch(const char *what);              // hipGetLastError() -> DF_ERR_LAUNCH
// Raises `kernel`'s dynamic-LDS limit (above the 64 KiB default) to `bytes` on the current device.  The attribute is per device (a process
// may drive several) and is set the first time a (device, kernel) pair is seen; safe to call from several host threads.  DF_OK, or
// DF_ERR_LAUNCH with the message recorded.
int raise_lds_limit(const void *kernel, int bytes);

// Development switches (A/B runs of kernel variants, verbose profiles) exist only in the DF_DEV build (libdfusion_hip_dev.so, compiled
// with -DDF_DEV and loaded by tests that compare variants): the shipped library reads no environment.
#ifdef DF_DEV
inline const char *dev_getenv(const char *name) { return getenv(name); }
#else
inline const char *dev_getenv(const char *) { return nullptr; }
#endif

inline hipStream_t to_stream(df_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int conv_out(int in, int k, int stride, int pad, int dil) { return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1; }

}  // namespace df
