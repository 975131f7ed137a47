// pano_angle.hpp -- a deterministic fp64 atan2 for the maps of reproject.hip, on the host and on the device.
// The maps need an angle per pixel; a device libm is not bit-equal to glibc's, and the maps are not separable, so the
// host-libm tables of the blend stage do not apply.  pano_atan2 therefore IS its definition: + - * / only, no contraction
// (every unit that includes this is built with -ffp-contract=off), so numpy float64 reproduces it bit for bit
// (tests/reproject_cases.py) and plain g++ builds it (tests/harness/reproject_harness.cc).
//   a = min(|x|, |y|) / max(|x|, |y|) in [0, 1];  k = round(8 a), c = k / 8;  t = (a - c) / (1 + a c), |t| <= 1/16;
//   atan(a) = atan(c) + atan(t) = T[k] + t (1 - s/3 + s^2/5 - ... - s^7/15), s = t^2: truncation <= (1/16)^17 / 17 = 2e-22;
//   then the octant: pi/2 - r where |y| > |x|, pi - r where x < 0, -r where y < 0.
// |pano_atan2 - atan2| <= 4e-15 rad is the contract (measured: DESIGN.md section 19).  x = y = 0 gives +0; the sign of a zero
// is not looked at (x = -0 counts as x >= 0); NaN in gives NaN out or a garbage angle, which the callers' bounds refuse.
#pragma once

#ifdef __HIPCC__
#define PANO_ANGLE_FN __host__ __device__ __forceinline__
#else
#define PANO_ANGLE_FN inline
#endif

#define PANO_PI 0x1.921fb54442d18p+1             /* M_PI */
#define PANO_PI_2 0x1.921fb54442d18p+0           /* M_PI / 2 */
#define PANO_2PI 0x1.921fb54442d18p+2            /* M_PI * 2 */

PANO_ANGLE_FN double pano_atan2(double y, double x) {
	const double ax = x < 0 ? -x : x, ay = y < 0 ? -y : y;
	if (ax == 0 && ay == 0) return 0.0;
	const double mn = ay > ax ? ax : ay, mx = ay > ax ? ay : ax;
	const double a = mn / mx;
	const int k = (int)(a * 8.0 + 0.5);                    // floor: the operand is >= 0
	const double c = (double)k * 0.125;
	const double t = (a - c) / (1.0 + a * c);
	const double s = t * t;
	double p = -0x1.1111111111111p-4;                      // -1/15
	p = p * s + 0x1.3b13b13b13b14p-4;                      //  1/13
	p = p * s - 0x1.745d1745d1746p-4;                      // -1/11
	p = p * s + 0x1.c71c71c71c71cp-4;                      //  1/9
	p = p * s - 0x1.2492492492492p-3;                      // -1/7
	p = p * s + 0x1.999999999999ap-3;                      //  1/5
	p = p * s - 0x1.5555555555555p-2;                      // -1/3
	p = p * s + 1.0;
	// atan(k / 8), correctly rounded.  A ladder rather than an indexed array: an array indexed per lane would live in scratch.
	const double T = k == 0 ? 0.0 : k == 1 ? 0x1.fd5ba9aac2f6ep-4 : k == 2 ? 0x1.f5b75f92c80ddp-3 : k == 3 ? 0x1.6f61941e4def1p-2
		: k == 4 ? 0x1.dac670561bb4fp-2 : k == 5 ? 0x1.1e00babdefeb4p-1 : k == 6 ? 0x1.4978fa3269ee1p-1
		: k == 7 ? 0x1.700a7c5784634p-1 : 0x1.921fb54442d18p-1;
	double r = T + t * p;
	if (ay > ax) r = PANO_PI_2 - r;
	if (x < 0) r = PANO_PI - r;
	if (y < 0) r = -r;
	return r;
}
