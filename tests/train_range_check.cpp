// Host check of mc-cnn_amd/csrc/train_range.h (tests/test_train_range_host.py builds it with -fsanitize=undefined,address
// -fno-sanitize-recover=all, so any signed overflow inside train_steps_fit ends the program): the limits of the four
// mc_train*_run entry points' range check, and agreement with a 128-bit restatement around every boundary.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../mc-cnn_amd/csrc/train_range.h"

typedef __int128 wide;
static const int64_t I64_MAX = INT64_MAX, I64_MIN = INT64_MIN;
static const int I32_MAX = INT32_MAX, I32_MIN = INT32_MIN;
static long n_checked = 0, n_failed = 0;

// the issue's five conditions, in arithmetic that cannot overflow because it is twice as wide
static bool fits128(int64_t t0, int n_steps, int n_pairs, int64_t n_perm)
{
	return n_perm >= 0 && n_steps >= 0 && n_pairs >= 1 && t0 >= 0 && t0 <= n_perm &&
	       (wide)t0 + (wide)n_steps * (wide)n_pairs <= (wide)n_perm;
}

// t0 + n_steps * n_pairs as the message prints it: exact where it fits int64_t, else the nearer end
static int64_t end128(int64_t t0, int n_steps, int n_pairs)
{
	const wide span = n_steps >= 0 && n_pairs >= 0 ? (wide)n_steps * (wide)n_pairs : 0;
	const wide e = (wide)t0 + span;
	return e > (wide)I64_MAX ? I64_MAX : e < (wide)I64_MIN ? I64_MIN : (int64_t)e;
}

static void check(int64_t t0, int n_steps, int n_pairs, int64_t n_perm)
{
	int64_t end = 12345;
	const bool got = mc::train_steps_fit(t0, n_steps, n_pairs, n_perm, &end);
	const bool plain = mc::train_steps_fit(t0, n_steps, n_pairs, n_perm);
	const bool want = fits128(t0, n_steps, n_pairs, n_perm);
	const int64_t want_end = end128(t0, n_steps, n_pairs);
	++n_checked;
	if (got != want || plain != want || end != want_end) {
		if (++n_failed <= 20)
			fprintf(stderr, "t0 %lld n_steps %d n_pairs %d n_perm %lld: got %d / %d, end %lld; want %d, end %lld\n", (long long)t0, n_steps,
			        n_pairs, (long long)n_perm, (int)got, (int)plain, (long long)end, (int)want, (long long)want_end);
	}
}

static void expect(bool want, int64_t t0, int n_steps, int n_pairs, int64_t n_perm)
{
	check(t0, n_steps, n_pairs, n_perm);
	if (mc::train_steps_fit(t0, n_steps, n_pairs, n_perm) != want) {
		++n_failed;
		fprintf(stderr, "t0 %lld n_steps %d n_pairs %d n_perm %lld: expected %d\n", (long long)t0, n_steps, n_pairs, (long long)n_perm, (int)want);
	}
}

static int64_t clamp64(wide v) { return v > (wide)I64_MAX ? I64_MAX : v < (wide)I64_MIN ? I64_MIN : (int64_t)v; }

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t next()   // splitmix64
{
	uint64_t z = (state += 0x9e3779b97f4a7c15ull);
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}

int main()
{
	// the last legal offset and one more (the message the GPU tests read: steps [12, 18) of 17 rows)
	expect(true, 11, 2, 3, 17);
	expect(false, 12, 2, 3, 17);
	int64_t end = 0;
	mc::train_steps_fit(12, 2, 3, 17, &end);
	if (end != 18) ++n_failed, fprintf(stderr, "end of [12, 18) is %lld\n", (long long)end);
	expect(true, 17, 0, 3, 17);     // no steps at the very end
	expect(false, 18, 0, 3, 17);    // t0 past the end, even with no steps
	expect(true, 0, 0, 1, 0);       // an empty permutation holds no step, and zero steps fit it
	expect(false, 0, 1, 1, 0);
	expect(false, 1, 0, 1, 0);
	expect(false, 0, 0, 1, -1);     // n_perm < 0
	expect(false, 0, 0, 1, I64_MIN);
	expect(false, -1, 0, 1, I64_MIN);
	expect(false, I64_MAX, 1, 1, I64_MIN);
	expect(false, -1, 1, 1, 17);
	expect(false, -1, 0, 1, 17);
	expect(false, I64_MIN, 2, 3, 17);
	expect(false, I64_MIN, I32_MAX, I32_MAX, I64_MAX);
	expect(false, 0, -1, 3, 17);
	expect(false, 0, I32_MIN, I32_MIN, 17);
	expect(false, 0, 1, 0, 17);
	expect(false, 0, 1, -1, 17);
	// t0 = 2^63 - 1 and 2^63 - 1 - k: the sum the old check formed wraps to a negative number that passed `<= n_perm`
	for (int k = 0; k <= 64; ++k) {
		for (int n_pairs : {1, 2, 3, 64, 1024, 4096}) {
			for (int n_steps : {0, 1, 2, 3, 256, I32_MAX}) {
				expect(false, I64_MAX - k, n_steps, n_pairs, 17);
				expect(false, I64_MAX - k, n_steps, n_pairs, 1 << 20);
				expect((int64_t)n_steps * n_pairs <= k, I64_MAX - k, n_steps, n_pairs, I64_MAX);
				expect(k >= 1 && (int64_t)n_steps * n_pairs <= k - 1, I64_MAX - k, n_steps, n_pairs, I64_MAX - 1);
			}
		}
	}
	mc::train_steps_fit(I64_MAX, 1, 1, 17, &end);
	if (end != I64_MAX) ++n_failed, fprintf(stderr, "the message's end is not saturated: %lld\n", (long long)end);
	// n_steps = 2^31 - 1 with n_pairs = 1024: the product needs 41 bits
	const int64_t big = (int64_t)I32_MAX * 1024;
	expect(true, 0, I32_MAX, 1024, big);
	expect(false, 0, I32_MAX, 1024, big - 1);
	expect(false, 1, I32_MAX, 1024, big);
	expect(true, 5, I32_MAX, 1024, big + 5);
	expect(true, I64_MAX - big, I32_MAX, 1024, I64_MAX);
	expect(false, I64_MAX - big + 1, I32_MAX, 1024, I64_MAX);
	expect(true, 0, I32_MAX, I32_MAX, (int64_t)I32_MAX * I32_MAX);
	expect(false, 0, I32_MAX, I32_MAX, (int64_t)I32_MAX * I32_MAX - 1);
	// random triples around the boundaries: n_perm near 0, near the span, near 2^63; t0 near 0, near n_perm - span, near n_perm, near 2^63
	const int steps_of[] = {0, 1, 2, 3, 255, 256, 65536, I32_MAX - 1, I32_MAX, -1, I32_MIN};
	const int pairs_of[] = {1, 2, 3, 64, 128, 256, 1024, 4096, I32_MAX, 0, -1, I32_MIN};
	for (int it = 0; it < 6000; ++it) {
		const int n_steps = steps_of[next() % 11], n_pairs = pairs_of[next() % 12];
		const int64_t span = n_steps >= 0 && n_pairs >= 0 ? (int64_t)n_steps * n_pairs : 0;
		const int64_t j1 = (int64_t)(next() % 9) - 4, j2 = (int64_t)(next() % 9) - 4;
		int64_t n_perm, t0;
		switch (next() % 5) {
		case 0: n_perm = j1; break;
		case 1: n_perm = span + j1; break;
		case 2: n_perm = I64_MAX - (int64_t)(next() % 9); break;
		case 3: n_perm = (int64_t)(next() >> 1); break;
		default: n_perm = (int64_t)(next() % ((uint64_t)1 << 40)); break;
		}
		switch (next() % 6) {
		case 0: t0 = j2; break;
		case 1: t0 = clamp64((wide)n_perm - span + j2); break;
		case 2: t0 = clamp64((wide)n_perm + j2); break;
		case 3: t0 = I64_MAX - (int64_t)(next() % 9); break;
		case 4: t0 = I64_MIN + (int64_t)(next() % 9); break;
		default: t0 = (int64_t)next(); break;
		}
		check(t0, n_steps, n_pairs, n_perm);
	}
	printf("%ld %ld\n", n_checked, n_failed);
	return n_failed ? 1 : 0;
}
