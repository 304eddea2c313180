// The range check of the four mc_train*_run entry points, asked by the run driver they share (run_steps, train_net.h): do
// the steps' rows [t0, t0 + n_steps * n_pairs) lie inside a permutation of n_perm rows?  Host code only, no HIP header, so
// that tests/train_range_check.cpp can compile it alone under the sanitizers.
#pragma once
#include <stdint.h>

namespace mc {

// True where n_perm >= 0, n_steps >= 0, n_pairs >= 1, 0 <= t0 <= n_perm and n_steps * n_pairs <= n_perm - t0.  No
// operation here can overflow for any argument: the product of two ints is below 2^62, and n_perm - t0 is formed only
// where 0 <= t0 <= n_perm.  *end, where given, receives t0 + n_steps * n_pairs for the caller's message, saturated at the
// ends of int64_t (and t0 itself where n_steps or n_pairs is negative): for arguments in range it is the exact sum.
inline bool train_steps_fit(int64_t t0, int n_steps, int n_pairs, int64_t n_perm, int64_t *end = nullptr)
{
	const int64_t span = n_steps >= 0 && n_pairs >= 0 ? (int64_t)n_steps * (int64_t)n_pairs : 0;
	if (end) *end = t0 > INT64_MAX - span ? INT64_MAX : t0 + span;   // span >= 0: only the upper end can be passed
	if (n_perm < 0 || n_steps < 0 || n_pairs < 1) return false;
	if (t0 < 0 || t0 > n_perm) return false;
	return span <= n_perm - t0;
}

}  // namespace mc
