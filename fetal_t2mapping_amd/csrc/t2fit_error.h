// t2fit_error.h -- error plumbing shared by the translation units of libt2fit_hip.so: the message
// t2fit_last_error() returns is one thread-local string whichever unit failed.  The string and the other basics of the
// library (ABI version, default configuration, device count) live in t2fit_host.hip.
#ifndef T2FIT_ERROR_H
#define T2FIT_ERROR_H

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/t2fit.h"

namespace t2fit {

// records `msg` as the calling thread's last error and returns `code` (defined in t2fit_host.hip)
int fail(int code, const std::string& msg);

}  // namespace t2fit

#define T2_HIP(call)                                                                            \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return t2fit::fail(T2FIT_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
  } while (0)

#endif  // T2FIT_ERROR_H
