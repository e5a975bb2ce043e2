// amp_sam.hpp -- what amp_sam.hip (the device codec for SAM text) needs from the ctx of amplihip.hip
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/amplihip.h"

namespace amp {

hipStream_t ctx_stream(const amp_ctx *ctx);      // the stream all work of the ctx runs on
int ctx_device(const amp_ctx *ctx);

}  // namespace amp
