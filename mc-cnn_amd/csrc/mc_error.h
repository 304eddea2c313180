// Error reporting of libmcadcensus.so, libmctrain.so and libmctrainslow.so (error.hip, linked into each: every library has its own
// thread-local message).  No HIP header: plain C++ units (hostio.cpp) include this too.
#pragma once
#include "../../include/mc_adcensus.h"

namespace mc {

void set_error(const char *fmt, ...);
int check_launch(const char *what);  // hipPeekAtLastError -> rc, like checkCudaError (adcensus.cu:31-36); clears the sticky error it reports
const char *last_error();            // the calling thread's message: mc_last_error / mc_train_last_error

#define MC_REQUIRE(cond, ...)                 \
	do {                                      \
		if (!(cond)) {                        \
			mc::set_error(__VA_ARGS__);       \
			return MC_EINVAL;                 \
		}                                     \
	} while (0)

}  // namespace mc
