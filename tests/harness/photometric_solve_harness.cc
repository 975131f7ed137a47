// photometric_solve_harness.cc -- the host-only units of the blend stage (csrc/photometric_solve.cc, csrc/blend_geom.cc) as a
// program of its own, for the sanitizers: the solvers index dense m x m matrices by hand from caller-supplied n, bx, by.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include -I csrc
//       photometric_solve_harness.cc csrc/photometric_solve.cc csrc/blend_geom.cc
// Checks return codes (and, for a refusal, which one) and that every output is finite; the numbers themselves are checked
// by tests/test_gain_solve_cpu.py, test_gain_block_solve_cpu.py, test_vignette_solve_cpu.py and test_blend_host_cpu.py.
#include "blend_shared.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static std::string g_error;
void op_set_error(const std::string& msg) { g_error = msg; }

static int g_checks = 0;
#define EXPECT(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); exit(1); } } while (0)
static bool refused_with(int rc, int code, const char* what) { return rc == code && g_error.find(what) != std::string::npos; }
template <typename T> static bool finite(const T* p, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false; return true; }

static std::mt19937_64 rng(20240917);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }

// ---------------------------------------------------- gains ----------------------------------------------------
// graph: 0 every pair overlaps, 1 images 0 and n - 1 are isolated, 2 no overlap at all
static void fill_gain_stats(int n, int B, int graph, std::vector<int64_t>& count, std::vector<int64_t>& sums) {
	const long long P = (long long)n * (n - 1) / 2, B2 = (long long)B * B;
	count.assign(P * B2, 0); sums.assign(6 * P * B2, 0);
	for (int a = 0; a < n; ++a)
		for (int b = a + 1; b < n; ++b) {
			if (graph == 2 || (graph == 1 && (a == 0 || b == n - 1))) continue;
			for (long long e = pair_index(a, b, n) * B2; e < (pair_index(a, b, n) + 1) * B2; ++e) {
				if (B > 1 && uni(0, 1) < 0.5) continue;          // a block pair without samples
				count[e] = 1 + (int64_t)uni(0, 4000);
				for (int q = 0; q < 6; ++q) sums[6 * e + q] = llrint(uni(0.05, 0.95) * (double)count[e] * GAIN_FIX);
			}
		}
}

static void gains() {
	std::vector<int64_t> count, sums;
	const int ns[4] = {1, 2, 5, 17};
	const int blocks[2][2] = {{1, 1}, {3, 2}};
	for (int n : ns)
		for (int graph = 0; graph < 3; ++graph)
			for (int pc = 0; pc < 2; ++pc) {
				fill_gain_stats(n, 1, graph, count, sums);
				std::vector<float> g(3 * (size_t)n, NAN);
				EXPECT(op_gain_solve(n, count.data(), sums.data(), 10.0 / 255.0, 0.1, pc, g.data()) == OP_OK);
				EXPECT(finite(g.data(), g.size()));
				if (graph == 2 || n == 1) for (float v : g) EXPECT(v == 1.f);
				for (const auto& bb : blocks) {
					const int B = bb[0] * bb[1];
					fill_gain_stats(n, B, graph, count, sums);
					std::vector<float> gb(3 * (size_t)n * B, NAN);
					EXPECT(op_gain_block_solve(n, bb[0], bb[1], count.data(), sums.data(), 10.0 / 255.0, 0.1, 0.1, pc, gb.data()) == OP_OK);
					EXPECT(finite(gb.data(), gb.size()));
				}
			}
	for (int pc = 0; pc < 2; ++pc) {                     // the finest grid, two images: 512 unknowns
		fill_gain_stats(2, 256, 0, count, sums);
		std::vector<float> gb(3 * 2 * 256, NAN);
		EXPECT(op_gain_block_solve(2, 16, 16, count.data(), sums.data(), 10.0 / 255.0, 0.1, 0.1, pc, gb.data()) == OP_OK);
		EXPECT(finite(gb.data(), gb.size()));
	}
	{	// the largest accepted size, n bx by == GAIN_BLOCK_MAX_UNKNOWNS: 16 images of 16 x 16 blocks, 120 x 65536 entries.  Only the
		// first and the last pair overlap (1024 unknowns in the dense solve), so both ends of every table are indexed.
		const int n = 16, B = 256;
		EXPECT((long long)n * B == GAIN_BLOCK_MAX_UNKNOWNS);
		const long long P = (long long)n * (n - 1) / 2, B2 = (long long)B * B;
		count.assign(P * B2, 0); sums.assign(6 * P * B2, 0);
		for (long long p : {0ll, P - 1})
			for (long long e = p * B2; e < (p + 1) * B2; e += 7) {
				count[e] = 1 + (int64_t)uni(0, 4000);
				for (int q = 0; q < 6; ++q) sums[6 * e + q] = llrint(uni(0.05, 0.95) * (double)count[e] * GAIN_FIX);
			}
		count[P * B2 - 1] = 5;                          // the very last entry
		for (int q = 0; q < 6; ++q) sums[6 * (P * B2 - 1) + q] = llrint(0.5 * 5 * GAIN_FIX);
		std::vector<float> gb(3 * (size_t)n * B, NAN);
		EXPECT(op_gain_block_solve(n, 16, 16, count.data(), sums.data(), 10.0 / 255.0, 0.1, 0.1, 0, gb.data()) == OP_OK);
		EXPECT(finite(gb.data(), gb.size()));
	}
	{	// one over: refused before anything is read or allocated -- the tables here hold ONE element each
		int64_t one_count = 1, one_sum = 1; float one_gain = 0.f;
		const int rc = op_gain_block_solve((int)GAIN_BLOCK_MAX_UNKNOWNS + 1, 1, 1, &one_count, &one_sum, 10.0 / 255.0, 0.1, 0.1, 0, &one_gain);
		EXPECT(refused_with(rc, OP_ERR_UNSUPPORTED, "exceed the dense solve's"));
		EXPECT(one_gain == 0.f);
	}
}

// --------------------------------------------------- vignette ---------------------------------------------------
// The moments of `samples` observations per overlapping pair of the exact model Y = e_k V(rho) L, V = 1 + a1 rho, rho in
// [0, rho_max], as include/openpano_hip.h states them.  Views form a chain: pair (a, a + 1) overlaps.
static void model_moments(int n, double a1, double rho_max, int samples, std::vector<int64_t>& count, std::vector<int64_t>& mom) {
	const long long P = (long long)n * (n - 1) / 2;
	count.assign(P, 0); mom.assign(VIG_MOMENTS * P, 0);
	std::vector<double> e(n);
	for (double& v : e) v = uni(0.7, 1.0);
	for (int a = 0; a + 1 < n; ++a) {
		const long long p = pair_index(a, a + 1, n);
		int64_t* m = mom.data() + VIG_MOMENTS * p;
		for (int s = 0; s < samples; ++s) {
			const float ra = (float)uni(0, rho_max), rb = (float)uni(0, rho_max);
			const double L = uni(0.2, 0.9);
			const double Ya = (float)(e[a] * (1.0 + a1 * ra) * L), Yb = (float)(e[a + 1] * (1.0 + a1 * rb) * L);
			double pa[7] = {1}, pb[7] = {1};
			for (int k = 1; k < 7; ++k) { pa[k] = pa[k - 1] * ra; pb[k] = pb[k - 1] * rb; }
			for (int k = 0; k < 7; ++k) { m[k] += llrint((Ya * Ya) * pb[k] * GAIN_FIX); m[7 + k] += llrint((Yb * Yb) * pa[k] * GAIN_FIX); }
			for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m[14 + 4 * i + j] += llrint(((Ya * Yb) * pa[i]) * pb[j] * GAIN_FIX);
		}
		count[p] = samples;
	}
}

static void vignette() {
	std::vector<int64_t> count, mom;
	const int ns[3] = {1, 2, 6};
	for (int n : ns)
		for (int degree = 1; degree <= 3; ++degree) {
			// the exact model with a mild curve: solved
			model_moments(n, -0.3, 1.0, 400, count, mom);
			std::vector<float> g(3 * (size_t)n, NAN); float poly[3] = {NAN, NAN, NAN};
			EXPECT(op_vignette_solve(n, count.data(), mom.data(), degree, 10.0 / 255.0, 1.0, 100.0, g.data(), poly) == OP_OK);
			EXPECT(finite(g.data(), g.size()) && finite(poly, 3));
			if (n == 1) continue;
			// noise -- moments that no set of samples produces: solved or refused, whichever; the outputs stay finite
			for (int64_t& v : mom) v = llrint(uni(0, 1) * 400 * GAIN_FIX);
			const int rc = op_vignette_solve(n, count.data(), mom.data(), degree, 10.0 / 255.0, 1.0, 100.0, g.data(), poly);
			EXPECT(rc == OP_OK || rc == OP_ERR_INVALID || rc == OP_ERR_UNSUPPORTED);
			EXPECT(finite(g.data(), g.size()) && finite(poly, 3));
			// refusal 1, "gain system not positive definite": the exact model's moments with A_0 of the first pair negated --
			// the first diagonal entry of the first round's gain system, -A_0 / sigma_n^2 + N / sigma_g^2, is negative
			model_moments(n, -0.3, 1.0, 400, count, mom);
			mom[0] = -mom[0];
			EXPECT(refused_with(op_vignette_solve(n, count.data(), mom.data(), degree, 10.0 / 255.0, 1.0, 100.0, g.data(), poly),
			                    OP_ERR_INVALID, "gain system not positive definite"));
			// refusal 2, "curve system not positive definite": the exact model's moments with C_11 of the first pair a thousand
			// times N -- the first round's gain system (A_0, B_0, C_00) is untouched, the curve system's first diagonal entry
			// g_a^2 A_2 - 2 g_a g_b C_11 + g_b^2 B_2 is negative
			model_moments(n, -0.3, 1.0, 400, count, mom);
			mom[14 + 4 * 1 + 1] = llrint(1000.0 * 400 * GAIN_FIX);
			EXPECT(refused_with(op_vignette_solve(n, count.data(), mom.data(), degree, 10.0 / 255.0, 1.0, 100.0, g.data(), poly),
			                    OP_ERR_INVALID, "curve system not positive definite"));
			// refusal 3, "curve not positive": the exact model with V = 1 - 1.2 rho observed on rho <= 0.8, where it is still
			// positive; the fit recovers a1 near -1.2, and V(1) < 0
			model_moments(n, -1.2, 0.8, 400, count, mom);
			EXPECT(refused_with(op_vignette_solve(n, count.data(), mom.data(), degree, 10.0 / 255.0, 1.0, 100.0, g.data(), poly),
			                    OP_ERR_UNSUPPORTED, "fitted curve is not positive"));
			for (float v : g) EXPECT(v == 1.f);            // a refusal leaves the neutral outputs
		}
}

// --------------------------------------------------- geometry ---------------------------------------------------
static op_config config() {
	op_config c; memset(&c, 0, sizeof(c));
	c.MAX_OUTPUT_SIZE = 8000; c.FOCAL_LENGTH = 37.f; c.GAUSS_WINDOW_FACTOR = 6;
	return c;
}

static void geometry() {
	const op_config cfg = config();
	const int n = 4, shapes[8] = {400, 300, 400, 300, 380, 310, 401, 299};
	for (int method = 0; method < 3; ++method) {
		double homo[9 * n];
		for (int i = 0; i < n; ++i) {
			double* h = homo + 9 * i;
			if (method == 0) { const double t[9] = {1, 0.01 * i, 250.0 * i, -0.01 * i, 1, 7.0 * i, 0, 0, 1}; memcpy(h, t, sizeof(t)); }
			else {           // a camera of focal length 500 turned by 0.3 i about the vertical axis
				const double c = std::cos(0.3 * i), s = std::sin(0.3 * i), f = 500;
				const double t[9] = {c, 0, s * f, 0, 1, 0, -s, 0, c * f}; memcpy(h, t, sizeof(t));
			}
		}
		op_blend_geom g; double hinv[9 * n], ranges[4 * n];
		EXPECT(op_blend_prepare(&cfg, method, 1, n, shapes, homo, &g, hinv, ranges) == OP_OK);
		EXPECT(finite(hinv, 9 * n) && finite(ranges, 4 * n) && finite(g.proj_min, 2) && finite(g.proj_max, 2) && finite(g.resolution, 2));
		EXPECT(g.resolution[0] > 0 && g.resolution[1] > 0);
		op_blend_image imgs[n]; memset(imgs, 0, sizeof(imgs));
		for (int i = 0; i < n; ++i) memcpy(imgs[i].range, ranges + 4 * i, sizeof(imgs[i].range));
		int H = -1, W = -1;
		EXPECT(op_blend_canvas_dims(&g, imgs, n, &H, &W) == OP_OK);
		EXPECT(H > 0 && W > 0 && H <= 80000 && W <= 80000);
		if (method == 0) {
			double bad[9 * n]; memcpy(bad, homo, sizeof(bad));
			memcpy(bad + 9 * 2 + 6, bad + 9 * 2, 3 * sizeof(double));        // image 2: third row = first row, singular
			EXPECT(refused_with(op_blend_prepare(&cfg, 0, 1, n, shapes, bad, &g, hinv, ranges), OP_ERR_INVALID, "homography 2 is not invertible"));
			memcpy(bad, homo, sizeof(bad));
			bad[9 * 3 + 2] = 1e7;                                             // image 3 ten million pixels away
			EXPECT(refused_with(op_blend_prepare(&cfg, 0, 1, n, shapes, bad, &g, hinv, ranges), OP_ERR_INVALID, "Target size too large"));
		}
	}
	EXPECT(refused_with(op_blend_canvas_dims(nullptr, nullptr, 0, nullptr, nullptr), OP_ERR_INVALID, "bad argument"));

	int nw = 0, nh = 0; double off[2] = {NAN, NAN};
	EXPECT(op_cyl_warp_shape(&cfg, 401, 299, 1.0, nullptr, 0, &nw, &nh, off) == OP_OK);
	EXPECT(nw > 0 && nh > 0 && finite(off, 2));
	std::vector<double> pts(2 * 33);
	for (size_t k = 0; k < pts.size(); k += 2) { pts[k] = uni(-200, 200); pts[k + 1] = uni(-150, 150); }
	int nw2 = 0, nh2 = 0;
	EXPECT(op_cyl_warp_shape(&cfg, 401, 299, 1.0, pts.data(), 33, &nw2, &nh2, off) == OP_OK);
	EXPECT(nw2 == nw && nh2 == nh && finite(pts.data(), pts.size()));
	EXPECT(refused_with(op_cyl_warp_shape(&cfg, 1, 299, 1.0, nullptr, 0, &nw, &nh, off), OP_ERR_INVALID, "bad argument"));

	BlurTaps t; memset(&t, 0, sizeof(t));
	EXPECT(gauss_taps(4.f, 15, t) == 0 && t.center == OP_MAX_KCENTER);       // 31 taps: the widest accepted kernel
	EXPECT(finite(t.k, 2 * OP_MAX_KCENTER + 1) && t.k[0] > 0 && t.k[2 * OP_MAX_KCENTER] > 0);
	EXPECT(gauss_taps(4.f, 16, t) == -1);                                     // 33 taps: refused before a tap is written
	for (int level = 0; level < 6; ++level) EXPECT(gauss_taps((float)(std::sqrt(level * 2 + 1.0) * 4), cfg.GAUSS_WINDOW_FACTOR, t) == 0);
}

int main() {
	gains();
	vignette();
	geometry();
	printf("photometric_solve_harness: %d checks passed\n", g_checks);
	return 0;
}
