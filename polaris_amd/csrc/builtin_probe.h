// builtin_probe.h -- what the device self-test of include/polaris_math.h (polaris_hip_selftest_builtins, kernels.h
// k_builtin_sweep) and its CPU side (oracle/polaris_oracle.cpp, polaris_oracle_builtins) both evaluate: ONE table of the
// built-ins the kernels call, ONE input generator, ONE fingerprint.  The two sides run the same calls on the same inputs, so
// a difference between them is a difference between the compilers' builds of polaris_math.h (a dropped flag, a contraction,
// a flushed denormal), not between two statements of the test.
//
// Inputs of function fn are numbered i = 0 .. pb_inputs(fn) - 1:
//   unary     x = the binary32 value with bit pattern i: all 2^32 patterns;
//   binary / ternary   i < PB_EDGES^3: the edge grid (x, y, z) = edge[i % E], edge[i / E % E], edge[i / E^2]; above it
//             2^28 counter-based draws, half of them raw bit patterns, half "ordinary" magnitudes (|x|, |y| < 4, z in [0, 1)).
// The result of input i is 32 bits (a float's bits, NaN canonicalised to 0x7fc00000: any NaN equals any NaN; the
// tone-map byte zero-extended).  The fingerprint of a chunk of 2^20 consecutive inputs is the wrapping 64-bit sum of
// pb_mix64(i, result) over the chunk, kept apart for inputs inside and outside the function's domain (pb_in_domain): a
// sum does not depend on order, so the device may add with atomics.
//
// Plain C++ with PM_HD functions only: no HIP types, no host library calls.
#pragma once

#include <stdint.h>

#include "polaris_math.h"

enum PbFn : uint32_t {
	PB_SQRT, PB_RCP, PB_FLOOR, PB_FABS, PB_SIGN, PB_SIN, PB_COS, PB_ATAN, PB_ACOS, PB_LOG, PB_EXP,
	PB_POW_GAMMA,   // pm_pow(x, 1 / 2.2f): the tone-mapper's call
	PB_U2F,         // (float)(uint32_t)i: the PRNG's conversion
	PB_TONEMAP,     // the tone-mapper's byte of one channel c (k_tonemap: weight and exposure already applied)
	PB_NUM_UNARY,
	PB_ATAN2 = PB_NUM_UNARY, PB_POW, PB_DIVIDE, PB_MIN, PB_MAX, PB_FMIN, PB_FMAX, PB_CLAMP, PB_MIX,
	PB_NUM_FN
};

#define PB_CHUNK_LOG2 20
#define PB_DRAWS (1ull << 28)
#define PB_EDGES 24u

// The edge grid of tests/tools/builtin_sweep.cpp: zeros, subnormals, 1 +- ulp, FLT_MAX, infinities, NaNs, pi, 2^-24, 2^23, 2^24.
PM_HD uint32_t pb_edge(uint32_t k) {
	switch (k) {
	case 0: return 0x00000000u;  case 1: return 0x80000000u;  case 2: return 0x00000001u;  case 3: return 0x80000001u;
	case 4: return 0x007fffffu;  case 5: return 0x00800000u;  case 6: return 0x80800000u;  case 7: return 0x3f800000u;
	case 8: return 0xbf800000u;  case 9: return 0x3f7fffffu;  case 10: return 0x3f800001u; case 11: return 0x7f7fffffu;
	case 12: return 0xff7fffffu; case 13: return 0x7f800000u; case 14: return 0xff800000u; case 15: return 0x7fc00000u;
	case 16: return 0xffc00000u; case 17: return 0x3f000000u; case 18: return 0x40000000u; case 19: return 0x40490fdbu;
	case 20: return 0xc0490fdbu; case 21: return 0x33800000u; case 22: return 0x4b000000u; default: return 0x4b800000u;
	}
}

PM_HD uint64_t pb_inputs(uint32_t fn) { return fn < PB_NUM_UNARY ? (1ull << 32) : (uint64_t)PB_EDGES * PB_EDGES * PB_EDGES + PB_DRAWS; }

PM_HD uint64_t pb_splitmix(uint64_t z) {
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// Input i of function fn (y, z = 0 for unary functions).
PM_HD void pb_input(uint32_t fn, uint64_t i, float &x, float &y, float &z) {
	if (fn < PB_NUM_UNARY) {
		x = pm_u2f((uint32_t)i);
		y = z = 0.0f;
		return;
	}
	const uint64_t E = PB_EDGES;
	if (i < E * E * E) {
		x = pm_u2f(pb_edge((uint32_t)(i % E)));
		y = pm_u2f(pb_edge((uint32_t)(i / E % E)));
		z = pm_u2f(pb_edge((uint32_t)(i / (E * E))));
		return;
	}
	const uint64_t k = i - E * E * E;
	const uint64_t r0 = pb_splitmix(0x1234567ull + (k + 1) * 0x9E3779B97F4A7C15ull);
	const uint64_t r1 = pb_splitmix(0x89ABCDEFull + (k + 1) * 0xD1B54A32D192ED03ull);
	if (k & 1) { // int -> float is correctly rounded on both sides, the scale by 2^-29 / 2^-32 exact
		x = (float)(int32_t)(uint32_t)r0 * 1.86264514923095703125e-9f;
		y = (float)(int32_t)(uint32_t)(r0 >> 32) * 1.86264514923095703125e-9f;
		z = (float)(uint32_t)r1 * 2.3283064365386962890625e-10f;
	} else {
		x = pm_u2f((uint32_t)r0);
		y = pm_u2f((uint32_t)(r0 >> 32));
		z = pm_u2f((uint32_t)r1);
	}
}

// Where the kernels may call the function (the domains polaris_math.h documents).  Outside, host and device could legally
// differ: pm__reduce_pio4 converts |x| * 4 / pi to uint32_t (undefined from ~3.4e9 on, and for NaN), pm_exp converts its
// argument to int32_t (undefined for NaN), the tone-map byte converts NaN to an integer.  The fingerprints keep those inputs
// apart, so a difference is reported on its side of the domain.
PM_HD bool pb_in_domain(uint32_t fn, float x, float y) {
	switch (fn) {
	case PB_SIN: case PB_COS: return pm_fabs(x) < 8192.0f;
	case PB_LOG: return x > 0.0f && x <= PM_FLT_MAX;
	case PB_EXP: return x == x;
	case PB_POW_GAMMA: case PB_TONEMAP: return x >= 0.0f;
	case PB_POW: return x >= 0.0f && pm_fabs(y) <= PM_FLT_MAX;
	default: return true;
	}
}

PM_HD uint32_t pb_canonical(float r) { return r != r ? 0x7fc00000u : pm_f2u(r); }

// The result bits of input (x, y, z) of fn; tonemap(c) is the caller's tone-map byte.
template <class Tonemap>
PM_HD uint32_t pb_eval(uint32_t fn, uint64_t i, float x, float y, float z, Tonemap tonemap) {
	switch (fn) {
	case PB_SQRT: return pb_canonical(pm_sqrt(x));
	case PB_RCP: return pb_canonical(pm_rcp(x));
	case PB_FLOOR: return pb_canonical(pm_floor(x));
	case PB_FABS: return pb_canonical(pm_fabs(x));
	case PB_SIGN: return pb_canonical(pm_sign(x));
	case PB_SIN: return pb_canonical(pm_sin(x));
	case PB_COS: return pb_canonical(pm_cos(x));
	case PB_ATAN: return pb_canonical(pm_atan(x));
	case PB_ACOS: return pb_canonical(pm_acos(x));
	case PB_LOG: return pb_canonical(pm_log(x));
	case PB_EXP: return pb_canonical(pm_exp(x));
	case PB_POW_GAMMA: return pb_canonical(pm_pow(x, 1.0f / 2.2f));
	case PB_U2F: return pb_canonical((float)(uint32_t)i);
	case PB_TONEMAP: return (uint32_t)tonemap(x);
	case PB_ATAN2: return pb_canonical(pm_atan2(x, y));
	case PB_POW: return pb_canonical(pm_pow(x, y));
	case PB_DIVIDE: return pb_canonical(x / y);
	case PB_MIN: return pb_canonical(pm_min(x, y));
	case PB_MAX: return pb_canonical(pm_max(x, y));
	case PB_FMIN: return pb_canonical(pm_fmin(x, y));
	case PB_FMAX: return pb_canonical(pm_fmax(x, y));
	case PB_CLAMP: return pb_canonical(pm_clamp(x, y, z));
	default: return pb_canonical(pm_mix(x, y, z));
	}
}

// What input i with result bits r adds to its chunk's fingerprint: an injective packing of (i, r), i < 2^32, through the
// splitmix64 finaliser (a bijection).
PM_HD uint64_t pb_mix64(uint64_t i, uint32_t r) { return pb_splitmix((i << 32) | r); }
