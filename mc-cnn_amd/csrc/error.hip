// The thread-local error message behind mc_last_error / mc_train_last_error (mc_error.h).
#include "mc_common.h"

#include <stdarg.h>

namespace mc {

static thread_local char g_err[512] = "";

const char *last_error() { return g_err; }

void set_error(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}

int check_launch(const char *what)
{
	const hipError_t e = hipPeekAtLastError();
	if (e != hipSuccess) {
		(void)hipGetLastError();
		set_error("%s: %s", what, hipGetErrorString(e));
		return (int)e;
	}
	return 0;
}

}  // namespace mc
