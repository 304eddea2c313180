// libmcsgmrecompute.so: the two kernels of the fused SGM schedule's recomputing vertical launches (sgm_line.h: sgm_line with MODE 4 and
// sgm_updown_line), a library of their own so that libmcadcensus.so's kernel set stays as it is.  libmcadcensus.so links against it;
// sgm_sweeps_ck (sgm.hip) decides when they run and builds their arguments.
#include "sgm_line.h"

#pragma GCC visibility push(default)
extern "C" int mc_sgm_recompute_launch(const mc::SgmPassArgs *A, size_t bytes, int which, hipStream_t st)
{
	using namespace mc;
	if (!A || bytes != sizeof(SgmPassArgs) || which < 0 || which > 2) return MC_EINVAL;
	// one wave per column of every volume
	const dim3 grid(cdiv((int64_t)A->nvol * A->W, 4)), block(256);
	if (which == 0) hipLaunchKernelGGL((sgm_pass_kernel<2, 4, 4, false, true, SGM_U_CK, false, false>), grid, block, 0, st, *A);
	else if (which == 1) hipLaunchKernelGGL((sgm_updown_kernel<SGM_CK_ROWS, false>), grid, block, 0, st, *A);
	else hipLaunchKernelGGL((sgm_updown_kernel<SGM_CK_ROWS, true>), grid, block, 0, st, *A);
	return 0;
}
#pragma GCC visibility pop
