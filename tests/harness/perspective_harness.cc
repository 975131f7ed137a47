// perspective_harness.cc -- the host geometry of cylinder mode's perspective correction (op_perspective_homography,
// csrc/blend_geom.cc) as a program of its own, for the sanitizers; and the pass itself on one host thread
// (perspective_host, the C++ twin of tests/perspective_cases.py's perspective_ref), which scripts/cylinder_probe.py times.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include -I csrc
//       perspective_harness.cc csrc/blend_geom.cc
//   perspective_harness                 the checks
//   perspective_harness --time H W N    N host passes over a synthetic H x W canvas; prints the milliseconds of the fastest
// Checks return codes (and, for a refusal, which one), that inv maps corners_std onto the corners, and that the host pass keeps
// to its buffers; the numbers themselves are checked by tests/test_perspective_cpu.py.
#include "blend_shared.hpp"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static std::string g_error;
void op_set_error(const std::string& msg) { g_error = msg; }

static int g_checks = 0;
#define EXPECT(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); exit(1); } } while (0)
static bool refused_with(int rc, const char* what) { return rc == OP_ERR_INVALID && g_error.find(what) != std::string::npos; }

// interpolate (lib/imgproc.cc:135-156); false = Color::NO
static bool interpolate(const float* img, int rows, int cols, float r, float c, float (&out)[3]) {
	if (!(r >= 0.f && c >= 0.f && r < (float)(rows - 1) && c < (float)(cols - 1))) return false;
	const int fr = (int)std::floor(r), fc = (int)std::floor(c);
	r -= (float)fr; c -= (float)fc;
	const float* p00 = img + ((size_t)fr * cols + fc) * 3;
	const float* p10 = p00 + (size_t)cols * 3;
	if (p00[0] < 0 || p10[0] < 0 || p10[3] < 0 || p00[3] < 0) return false;
	const float w[4] = {(1 - r) * (1 - c), r * (1 - c), r * c, (1 - r) * c};
	const float* p[4] = {p00, p10, p10 + 3, p00 + 3};
	for (int ch = 0; ch < 3; ++ch) {
		float s = 0.f;
		for (int q = 0; q < 4; ++q) s += p[q][ch] * w[q];
		out[ch] = s;
	}
	return true;
}

// the LinearBlender pass of cylstitcher.cc:170-179 over one image, the canvas itself
static void perspective_host(const float* src, int H, int W, const double* d, int ordered_input, int lazy, float* out) {
	for (int i = 0; i < H; ++i)
		for (int j = 0; j < W; ++j) {
			const double rx = d[0] * j + d[1] * i + d[2] * 1.0, ry = d[3] * j + d[4] * i + d[5] * 1.0, rz = d[6] * j + d[7] * i + d[8] * 1.0;
			const double denom = 1.0 / rz;
			const double ox = rx * denom, oy = ry * denom;
			float s[3] = {0.f, 0.f, 0.f}, wsum = 0.f, col[3];
			if (!(ox < 0 || ox >= W || oy < 0 || oy >= H) && !std::isnan(ox)) {
				const float r = (float)oy, c = (float)ox;
				if (interpolate(src, H, W, r, c, col) && !(col[0] < 0)) {
					float w = (float)(0.5 - std::fabs((double)(c / (float)W) - 0.5));
					if (!ordered_input) w = (float)((double)w * (0.5 - std::fabs((double)(r / (float)H) - 0.5)));
					for (int ch = 0; ch < 3; ++ch) s[ch] += col[ch] * w;
					wsum += w;
				}
			}
			float* row = out + ((size_t)i * W + j) * 3;
			if (lazy ? wsum != 0.f : wsum > 0) {
				const float iw = (float)(1.0 / (double)wsum);
				for (int ch = 0; ch < 3; ++ch) row[ch] = lazy ? s[ch] / wsum : s[ch] * iw;
			} else row[0] = row[1] = row[2] = -1.f;
		}
}

static std::vector<float> synthetic(int H, int W) {
	std::vector<float> v((size_t)H * W * 3);
	unsigned x = 12345u;
	for (float& f : v) { x = x * 1664525u + 1013904223u; f = (float)(x >> 8) * (1.f / 16777216.f); }
	for (int j = 0; j < W; ++j) for (int ch = 0; ch < 3; ++ch) v[(size_t)j * 3 + ch] = -1.f;     // a Color::NO line
	return v;
}

struct Bundle { double proj_min[2]; int ref[2], first[2]; double fh[9]; int last[2]; double lh[9]; int canvas[2]; };

static int solve(const Bundle& b, double* inv, double* corners) {
	op_blend_geom g;
	memset(&g, 0, sizeof g);
	g.proj_min[0] = b.proj_min[0]; g.proj_min[1] = b.proj_min[1];
	return op_perspective_homography(&g, b.ref[0], b.ref[1], b.first[0], b.first[1], b.fh, b.last[0], b.last[1], b.lh, b.canvas[0], b.canvas[1], inv, corners);
}

static void geometry() {
	const Bundle good[3] = {
		{{-301.5, -203.25}, {600, 400}, {600, 400}, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {600, 400}, {1, -0.007, 431.7, 0.007, 1, 6.2, 1e-5, -2e-6, 1}, {1033, 412}},
		{{-1290.125, -260.5}, {640, 480}, {612, 470}, {1, 0.02, -872.4, -0.02, 1, 11.3, -3e-5, 4e-6, 1}, {655, 491}, {1, -0.014, 460.9, 0.014, 1, -7.7, 2e-5, 1e-6, 1}, {2101, 533}},
		{{-9480.75, -1410.5}, {4000, 3000}, {3000, 4000}, {-0.026, -1, -7400.2, 1, -0.026, 40.6, -4e-6, 1e-6, 1}, {4000, 3000}, {1, 0.012, 7613.4, -0.012, 1, -55.1, 3e-6, -5e-7, 1}, {18803, 3390}},
	};
	for (const Bundle& b : good) {
		double inv[9], corners[8], inv2[9];
		EXPECT(solve(b, inv, corners) == OP_OK);
		EXPECT(solve(b, inv2, nullptr) == OP_OK && memcmp(inv, inv2, sizeof inv) == 0);     // corners are optional
		EXPECT(inv[8] == 1.0);
		const double sx[4] = {0, 0, (double)b.canvas[0], (double)b.canvas[0]}, sy[4] = {0, (double)b.canvas[1], 0, (double)b.canvas[1]};
		for (int k = 0; k < 4; ++k) {
			const double z = inv[6] * sx[k] + inv[7] * sy[k] + inv[8];
			const double x = (inv[0] * sx[k] + inv[1] * sy[k] + inv[2]) / z, y = (inv[3] * sx[k] + inv[4] * sy[k] + inv[5]) / z;
			EXPECT(std::fabs(x - corners[2 * k]) < 1e-6 && std::fabs(y - corners[2 * k + 1]) < 1e-6);
		}
	}
	double inv[9], corners[8];
	Bundle b = good[0];
	EXPECT(refused_with(op_perspective_homography(nullptr, 1, 1, 1, 1, b.fh, 1, 1, b.lh, 1, 1, inv, corners), "bad argument"));
	{ op_blend_geom g; memset(&g, 0, sizeof g);
	  EXPECT(refused_with(op_perspective_homography(&g, 1, 1, 1, 1, nullptr, 1, 1, b.lh, 1, 1, inv, corners), "bad argument"));
	  EXPECT(refused_with(op_perspective_homography(&g, 1, 1, 1, 1, b.fh, 1, 1, nullptr, 1, 1, inv, corners), "bad argument"));
	  EXPECT(refused_with(op_perspective_homography(&g, 1, 1, 1, 1, b.fh, 1, 1, b.lh, 1, 1, nullptr, corners), "bad argument")); }
	// a zero-size view, reference view or canvas
	for (int which = 0; which < 8; ++which) {
		b = good[1];
		int* f[8] = {&b.ref[0], &b.ref[1], &b.first[0], &b.first[1], &b.last[0], &b.last[1], &b.canvas[0], &b.canvas[1]};
		*f[which] = 0;
		EXPECT(refused_with(solve(b, inv, corners), "a size below 1"));
		*f[which] = -3;
		EXPECT(refused_with(solve(b, inv, corners), "a size below 1"));
	}
	// collinear corners: every corner on one line; the two of one view in one point; three of the four on a line
	b = good[0];
	const double flat_first[9] = {1, 0, -300, 0, 0, 0, 0, 0, 1}, flat_last[9] = {1, 0, 300, 0, 0, 0, 0, 0, 1};
	memcpy(b.fh, flat_first, sizeof b.fh); memcpy(b.lh, flat_last, sizeof b.lh);
	EXPECT(refused_with(solve(b, inv, corners), "three corners on one line"));
	b = good[0];
	const double point[9] = {0, 0, -300, 0, 0, 0, 0, 0, 1};
	memcpy(b.fh, point, sizeof b.fh);
	EXPECT(refused_with(solve(b, inv, corners), "three corners on one line"));
	b = good[0];
	const double through[9] = {0, 0, 431.7 - 300, 0, 1, 6.2, 0, 0, 1};        // the first view's corners on the last view's right edge, about
	memcpy(b.fh, through, sizeof b.fh);
	const double upright[9] = {1, 0, 131.7 - 300, 0, 1, 6.2, 0, 0, 1};
	memcpy(b.lh, upright, sizeof b.lh);
	EXPECT(refused_with(solve(b, inv, corners), "three corners on one line"));
	// non-finite homographies and the corners they make
	const double bad[4] = {NAN, INFINITY, -INFINITY, std::numeric_limits<double>::max()};
	for (double v : bad)
		for (int k = 0; k < 9; ++k)
			for (int side = 0; side < 2; ++side) {
				b = good[1];
				(side ? b.lh : b.fh)[k] = v;
				const int rc = solve(b, inv, corners);
				EXPECT(rc == OP_OK || rc == OP_ERR_INVALID);
				if (rc == OP_OK) for (double e : inv) EXPECT(std::isfinite(e));
			}
	b = good[1];
	for (double& e : b.fh) e = 0;                          // z = 0: 0 / 0
	EXPECT(refused_with(solve(b, inv, corners), "a corner is not finite"));
}

static void pass() {
	const int shapes[5][2] = {{2, 2}, {1, 7}, {5, 257}, {37, 53}, {67, 130}};
	for (const auto& s : shapes) {
		const int H = s[0], W = s[1];
		const std::vector<float> src = synthetic(H, W);
		const double maps[5][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {1.02, 0.03, -0.4, 0.01, 0.98, 0.3, 0.05 / W, -0.03 / H, 1},
			{1, 0, (double)-(W / 2), 0, 1, 0.5, 1, 1, -(W / 2 + 1.0)}, {1, 0, 0.5, 0, 1, -1e-50, 0, 0, 1}, {1, 0, W + 3.0, 0, 1, 0, 0, 0, 1}};
		for (const auto& m : maps)
			for (int flags = 0; flags < 4; ++flags) {
				std::vector<float> out((size_t)H * W * 3, NAN);
				perspective_host(src.data(), H, W, m, flags & 1, flags >> 1, out.data());
				for (float v : out) EXPECT(v == -1.f || (v >= 0.f && v <= 1.0001f));
			}
	}
}

int main(int argc, char** argv) {
	if (argc == 5 && std::string(argv[1]) == "--time") {
		const int H = atoi(argv[2]), W = atoi(argv[3]), N = atoi(argv[4]);
		if (H < 1 || W < 1 || N < 1) return 2;
		const std::vector<float> src = synthetic(H, W);
		std::vector<float> out(src.size());
		const double m[9] = {1.02, 0.03, -0.4, 0.01, 0.98, 0.3, 0.05 / W, -0.03 / H, 1};
		double best = 1e300;
		for (int k = 0; k < N; ++k) {
			const auto t0 = std::chrono::steady_clock::now();
			perspective_host(src.data(), H, W, m, 1, 0, out.data());
			best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
		}
		printf("perspective_host: %d x %d, fastest of %d: %.3f ms (checksum %g)\n", H, W, N, best, (double)out[out.size() / 2]);
		return 0;
	}
	geometry();
	pass();
	printf("perspective_harness: %d checks passed\n", g_checks);
	return 0;
}
