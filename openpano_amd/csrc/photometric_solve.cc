// photometric_solve.cc -- the host solvers of the photometric corrections: gains (op_gain_solve), block gains
// (op_gain_block_solve) and the shared vignetting curve (op_vignette_solve) from the statistics of overlap.hip, and the
// checks of the tables the blend entry points take.  Plain C++ (no HIP), fp64 in a fixed order, built without contraction;
// tests/harness/photometric_solve_harness.cc runs it under the sanitizers.
#include "blend_shared.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

// The vignetting curve V(rho) = 1 + a1 rho + a2 rho^2 + a3 rho^3 (a: a1..a3) stays above VIG_MIN_CURVE on [0, 1]: its minimum
// there lies at rho = 0 (V = 1), rho = 1 or a root of V' inside, all checked in fp64.
constexpr double VIG_MIN_CURVE = 1e-6;
bool vignette_curve_positive(const double a[3]) {
	if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2])) return false;
	auto V = [&](double r) { return 1.0 + r * (a[0] + r * (a[1] + r * a[2])); };
	double cand[3] = {1.0, -1.0, -1.0};
	if (a[2] != 0.0) {                                  // V' = a1 + 2 a2 rho + 3 a3 rho^2
		const double disc = 4.0 * a[1] * a[1] - 12.0 * a[2] * a[0];
		if (disc >= 0.0) { const double sq = std::sqrt(disc); cand[1] = (-2.0 * a[1] + sq) / (6.0 * a[2]); cand[2] = (-2.0 * a[1] - sq) / (6.0 * a[2]); }
	} else if (a[1] != 0.0) cand[1] = -a[0] / (2.0 * a[1]);
	for (double r : cand)
		if (r >= 0.0 && r <= 1.0 && !(V(r) > VIG_MIN_CURVE)) return false;
	return true;
}

// the views of the vignetting entry points are in their own lens frame: a cylinder pre-warp -- a pixel buffer whose size
// (mat_h / mat_w, when set) differs from the ImageRef's -- is refused
int check_lens_frame(const char* who, const op_blend_image* imgs, int n) {
	for (int k = 0; k < n; ++k)
		if ((imgs[k].mat_h > 0 && imgs[k].mat_h != imgs[k].h) || (imgs[k].mat_w > 0 && imgs[k].mat_w != imgs[k].w))
			OP_FAIL(OP_ERR_UNSUPPORTED, std::string(who) + ": image " + std::to_string(k) + " is pre-warped (mat_h / mat_w set): its samples are not in the lens frame");
	return OP_OK;
}

// every gain of a host table (count floats, per_image of them per image; NULL: none) finite and positive
int check_gains(const char* who, const float* gains, long long count, long long per_image) {
	for (long long e = 0; gains && e < count; ++e)
		if (!std::isfinite(gains[e]) || !(gains[e] > 0.f))
			OP_FAIL(OP_ERR_INVALID, std::string(who) + ": gain " + std::to_string(e) + " (image " + std::to_string(e / per_image) + ") is not finite and positive");
	return OP_OK;
}

namespace {

// The dense solve of op_gain_solve and op_gain_block_solve: A = L L^T in place (lower triangle), then L y = rhs,
// L^T g = y; rhs receives g.  fp64, fixed loop order.  false: A is not positive definite.
bool gain_cholesky_solve(std::vector<double>& A, std::vector<double>& rhs, int m) {
	for (int j = 0; j < m; ++j) {
		double d = A[(size_t)j * m + j];
		for (int k = 0; k < j; ++k) d -= A[(size_t)j * m + k] * A[(size_t)j * m + k];
		if (!(d > 0)) return false;
		const double l = std::sqrt(d);
		A[(size_t)j * m + j] = l;
		for (int i = j + 1; i < m; ++i) {
			double v = A[(size_t)i * m + j];
			for (int k = 0; k < j; ++k) v -= A[(size_t)i * m + k] * A[(size_t)j * m + k];
			A[(size_t)i * m + j] = v / l;
		}
	}
	for (int i = 0; i < m; ++i) {
		double v = rhs[i];
		for (int k = 0; k < i; ++k) v -= A[(size_t)i * m + k] * rhs[k];
		rhs[i] = v / A[(size_t)i * m + i];
	}
	for (int i = m - 1; i >= 0; --i) {
		double v = rhs[i];
		for (int k = i + 1; k < m; ++k) v -= A[(size_t)k * m + i] * rhs[k];
		rhs[i] = v / A[(size_t)i * m + i];
	}
	return true;
}

// The active images of a solve -- those in a pair (a < b) for which overlaps(a, b, p) holds, p = pair_index(a, b, n), asked
// once per pair in pair order -- in index order; slot[k] is image k's place among them, -1 for the others.
template <typename F>
std::vector<int> active_images(int n, std::vector<int>& slot, F&& overlaps) {
	slot.assign(n, -1);
	for (int a = 0; a < n; ++a)
		for (int b = a + 1; b < n; ++b)
			if (overlaps(a, b, pair_index(a, b, n))) slot[a] = slot[b] = 0;
	std::vector<int> act;
	for (int a = 0; a < n; ++a) if (slot[a] == 0) { slot[a] = (int)act.size(); act.push_back(a); }
	return act;
}

// The normal equations of op_gain_block_solve (below) and their solve, after the entry point's own checks: op_gain_solve is
// the case bx = by = 1.  `who` prefixes the failure.
int gain_unit_solve(const char* who, int n, int bx, int by, const int64_t* count, const int64_t* sums, double sigma_n, double sigma_g,
		double sigma_s, int per_channel, float* gains) {
	const int B = bx * by;
	const long long B2 = (long long)B * B;
	// the active images, and M_k
	std::vector<double> M(n, 0.0);
	std::vector<int> slot;
	const std::vector<int> act = active_images(n, slot, [&](int a, int b, long long p) {
		int64_t N = 0;
		for (long long e = p * B2; e < (p + 1) * B2; ++e) N += count[e];
		if (N > 0) { M[a] += (double)N; M[b] += (double)N; }
		return N > 0;
	});
	const int m = (int)act.size() * B;
	for (long long e = 0; e < 3ll * n * B; ++e) gains[e] = 1.f;
	if (m == 0) return OP_OK;
	const double inv_n2 = 1.0 / (sigma_n * sigma_n), inv_g2 = 1.0 / (sigma_g * sigma_g), inv_s2 = 1.0 / (sigma_s * sigma_s);
	std::vector<double> A((size_t)m * m), rhs(m);
	const int nsolve = per_channel ? 3 : 1;
	for (int ch = 0; ch < nsolve; ++ch) {
		std::fill(A.begin(), A.end(), 0.0); std::fill(rhs.begin(), rhs.end(), 0.0);
		for (int a = 0; a < n; ++a)
			for (int b = a + 1; b < n; ++b) {
				const long long p = pair_index(a, b, n);
				for (int qa = 0; qa < B; ++qa)
					for (int qb = 0; qb < B; ++qb) {
						const long long e = p * B2 + (long long)qa * B + qb;
						if (count[e] <= 0) continue;
						const double N = (double)count[e], den = GAIN_FIX * N;
						const int64_t* S = sums + 6 * e;
						double Iab, Iba;
						if (per_channel) { Iab = (double)S[ch] / den; Iba = (double)S[3 + ch] / den; }
						else { Iab = ((double)(S[0] + S[1] + S[2]) / 3.0) / den; Iba = ((double)(S[3] + S[4] + S[5]) / 3.0) / den; }
						const int sa = slot[a] * B + qa, sb = slot[b] * B + qb;
						A[(size_t)sa * m + sa] += N * (2.0 * Iab * Iab * inv_n2 + inv_g2);
						A[(size_t)sb * m + sb] += N * (2.0 * Iba * Iba * inv_n2 + inv_g2);
						const double off = N * (2.0 * Iab * Iba * inv_n2);
						A[(size_t)sa * m + sb] -= off;
						A[(size_t)sb * m + sa] -= off;
						rhs[sa] += N * inv_g2;
						rhs[sb] += N * inv_g2;
					}
			}
		for (int s = 0; s < (int)act.size(); ++s) {       // smoothness: the grid Laplacian of every active image
			const double w = 2.0 * (M[act[s]] / B) * inv_s2;
			for (int v = 0; v < by; ++v)
				for (int u = 0; u < bx; ++u) {
					const int q = s * B + v * bx + u;
					for (int d = 0; d < 2; ++d) {
						if (d == 0 ? u + 1 >= bx : v + 1 >= by) continue;
						const int q2 = q + (d == 0 ? 1 : bx);
						A[(size_t)q * m + q] += w; A[(size_t)q2 * m + q2] += w;
						A[(size_t)q * m + q2] -= w; A[(size_t)q2 * m + q] -= w;
					}
				}
		}
		if (!gain_cholesky_solve(A, rhs, m)) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": system not positive definite (inconsistent statistics)");
		for (int s = 0; s < (int)act.size(); ++s)
			for (int q = 0; q < B; ++q) {
				const float gv = (float)rhs[(size_t)s * B + q];
				float* o = gains + 3 * ((long long)act[s] * B + q);
				if (per_channel) o[ch] = gv;
				else o[0] = o[1] = o[2] = gv;
			}
	}
	return OP_OK;
}

}	// namespace

extern "C" {

// Gain compensation (Brown & Lowe, IJCV 2007, section 6), host only: minimise
//   e = 1/2 sum_a sum_{b != a} N_ab [ (g_a I_ab - g_b I_ba)^2 / sigma_n^2 + (1 - g_a)^2 / sigma_g^2 ]
// through its normal equations (for every a, over b != a)
//   sum_b N_ab [ (2 I_ab^2 / sigma_n^2 + 1 / sigma_g^2) g_a - (2 I_ab I_ba / sigma_n^2) g_b ] = sum_b N_ab / sigma_g^2,
// I_ab = S_ab / (2^32 N_ab) the mean of image a over its overlap with b.  The matrix is symmetric and, for sigma_g > 0,
// positive definite on the images with any overlap; those without are g = 1 and left out.  Cholesky, fp64, fixed loop
// order: the gains are a function of the statistics alone.
int op_gain_solve(int n, const int64_t* count, const int64_t* sums, double sigma_n, double sigma_g, int per_channel, float* gains) {
	if (n < 1 || !gains || (n > 1 && (!count || !sums)) || !(sigma_n > 0) || !(sigma_g > 0) || !std::isfinite(sigma_n) || !std::isfinite(sigma_g) ||
			(per_channel != 0 && per_channel != 1))
		OP_FAIL(OP_ERR_INVALID, "op_gain_solve: bad argument");
	const long long npairs = (long long)n * (n - 1) / 2;
	for (long long p = 0; p < npairs; ++p)
		if (count[p] < 0) OP_FAIL(OP_ERR_INVALID, "op_gain_solve: negative overlap count at pair " + std::to_string(p));
	return gain_unit_solve("op_gain_solve", n, 1, 1, count, sums, sigma_n, sigma_g, 1.0, per_channel, gains);   // one unit per image: no edges
}

// Block gain compensation, host only: op_gain_solve's normal equations over units (k, q) -- entry e = p B^2 + qa B + qb
// couples unit (a, qa) with (b, qb) exactly as pair p couples a with b there, in the same pair order -- plus, for every
// 4-neighbour edge q ~ q' of an active image k, 2 lambda_k / sigma_s^2 on both diagonals and -2 lambda_k / sigma_s^2 off
// them, lambda_k = M_k / B, M_k = the overlap samples of k over all its pairs.  With B = 1 there are no edges: op_gain_solve.
int op_gain_block_solve(int n, int bx, int by, const int64_t* count, const int64_t* sums, double sigma_n, double sigma_g, double sigma_s,
		int per_channel, float* gains) {
	if (n < 1 || !gains || (n > 1 && (!count || !sums)) || bx < 1 || bx > GAIN_MAX_BLOCKS || by < 1 || by > GAIN_MAX_BLOCKS ||
			!(sigma_n > 0) || !(sigma_g > 0) || !(sigma_s > 0) || !std::isfinite(sigma_n) || !std::isfinite(sigma_g) || !std::isfinite(sigma_s) ||
			(per_channel != 0 && per_channel != 1))
		OP_FAIL(OP_ERR_INVALID, "op_gain_block_solve: bad argument");
	const long long B = (long long)bx * by, entries = (long long)n * (n - 1) / 2 * B * B;
	if (n * B > GAIN_BLOCK_MAX_UNKNOWNS)
		OP_FAIL(OP_ERR_UNSUPPORTED, "op_gain_block_solve: " + std::to_string(n * B) + " units (n bx by) exceed the dense solve's " +
		        std::to_string(GAIN_BLOCK_MAX_UNKNOWNS));
	for (long long e = 0; e < entries; ++e)
		if (count[e] < 0) OP_FAIL(OP_ERR_INVALID, "op_gain_block_solve: negative overlap count at entry " + std::to_string(e));
	return gain_unit_solve("op_gain_block_solve", n, bx, by, count, sums, sigma_n, sigma_g, sigma_s, per_channel, gains);
}

// Vignetting compensation, host only: gains g_k and one curve a = (1, a1, a2, a3) shared by all views minimising
//   E = sum_p [ (g_a^2 a'H(A)a - 2 g_a g_b a'Ca + g_b^2 a'H(B)a) / sigma_n^2 + N ((1 - g_a)^2 + (1 - g_b)^2) / sigma_g^2 ]
//     + (sum_p N) (a1^2 + a2^2 + a3^2) / sigma_v^2,
// the first term the sum over the pair's samples of (g_a Y_a V(rho_b) - g_b Y_b V(rho_a))^2 written with the moments
// (H(A) the Hankel matrix A_{i+j}, moments / 2^32).  Alternation from a = 0, each step a closed-form SPD solve: g given a
// (op_gain_solve's pattern, its Cholesky), then a1..a_degree given g (degree x degree); stop after VIG_MAX_ROUNDS rounds or
// when a round lowers E by no more than VIG_TOL E; then the gains are normalised to an overlap-weighted mean of 1.  fp64,
// fixed order: a function of the statistics alone.
constexpr int VIG_MAX_ROUNDS = 100;
constexpr double VIG_TOL = 1e-12;
int op_vignette_solve(int n, const int64_t* count, const int64_t* moments, int degree, double sigma_n, double sigma_g, double sigma_v,
		float* gains, float* poly) {
	if (n < 1 || !gains || !poly || (n > 1 && (!count || !moments)) || degree < 1 || degree > 3 || !(sigma_n > 0) || !(sigma_g > 0) ||
			!(sigma_v > 0) || !std::isfinite(sigma_n) || !std::isfinite(sigma_g) || !std::isfinite(sigma_v))
		OP_FAIL(OP_ERR_INVALID, "op_vignette_solve: bad argument");
	const long long npairs = (long long)n * (n - 1) / 2;
	for (long long p = 0; p < npairs; ++p)
		if (count[p] < 0) OP_FAIL(OP_ERR_INVALID, "op_vignette_solve: negative overlap count at pair " + std::to_string(p));
	for (int e = 0; e < 3 * n; ++e) gains[e] = 1.f;
	poly[0] = poly[1] = poly[2] = 0.f;
	// the pairs with overlap, in pair order, with their moments in [0, 1] units, and the active images
	struct VPair { int a, b; double N, A[7], B[7], C[16]; };
	std::vector<VPair> pairs;
	double Mtot = 0.0;
	std::vector<int> slot;
	const std::vector<int> act = active_images(n, slot, [&](int a, int b, long long p) {
		if (count[p] <= 0) return false;
		VPair v; v.a = a; v.b = b; v.N = (double)count[p];
		const int64_t* mo = moments + (long long)VIG_MOMENTS * p;
		for (int k = 0; k < 7; ++k) { v.A[k] = (double)mo[k] / GAIN_FIX; v.B[k] = (double)mo[7 + k] / GAIN_FIX; }
		for (int k = 0; k < 16; ++k) v.C[k] = (double)mo[14 + k] / GAIN_FIX;
		pairs.push_back(v);
		Mtot += v.N;
		return true;
	});
	const int m = (int)act.size();
	if (m == 0) return OP_OK;
	const double inv_n2 = 1.0 / (sigma_n * sigma_n), inv_g2 = 1.0 / (sigma_g * sigma_g), inv_v2 = 1.0 / (sigma_v * sigma_v);
	double a[4] = {1.0, 0.0, 0.0, 0.0};
	std::vector<double> g(n, 1.0);
	// a'Ma for the Hankel matrix of h, and for C (row: the power of rho_a)
	auto hank = [&](const double* h) { double t = 0.0; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) t += a[i] * a[j] * h[i + j]; return t; };
	auto cross = [&](const double* c) { double t = 0.0; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) t += a[i] * a[j] * c[4 * i + j]; return t; };
	auto energy = [&]() {
		double e = 0.0;
		for (const VPair& v : pairs) {
			const double ga = g[v.a], gb = g[v.b];
			e += (ga * ga * hank(v.A) - 2.0 * ga * gb * cross(v.C) + gb * gb * hank(v.B)) * inv_n2;
			e += v.N * ((1.0 - ga) * (1.0 - ga) + (1.0 - gb) * (1.0 - gb)) * inv_g2;
		}
		return e + Mtot * (a[1] * a[1] + a[2] * a[2] + a[3] * a[3]) * inv_v2;
	};
	std::vector<double> A((size_t)m * m), rhs(m);
	double e_prev = energy();
	for (int round = 0; round < VIG_MAX_ROUNDS; ++round) {
		// g given a
		std::fill(A.begin(), A.end(), 0.0); std::fill(rhs.begin(), rhs.end(), 0.0);
		for (const VPair& v : pairs) {
			const int sa = slot[v.a], sb = slot[v.b];
			A[(size_t)sa * m + sa] += hank(v.A) * inv_n2 + v.N * inv_g2;
			A[(size_t)sb * m + sb] += hank(v.B) * inv_n2 + v.N * inv_g2;
			const double off = cross(v.C) * inv_n2;
			A[(size_t)sa * m + sb] -= off;
			A[(size_t)sb * m + sa] -= off;
			rhs[sa] += v.N * inv_g2;
			rhs[sb] += v.N * inv_g2;
		}
		if (!gain_cholesky_solve(A, rhs, m)) OP_FAIL(OP_ERR_INVALID, "op_vignette_solve: gain system not positive definite (inconsistent statistics)");
		for (int i = 0; i < m; ++i) g[act[i]] = rhs[i];
		// a given g: Q = sum_p [g_a^2 H(A) - g_a g_b (C + C') + g_b^2 H(B)] / sigma_n^2, then
		// (Q[1.., 1..] + (sum N) / sigma_v^2 I) a' = -Q[1.., 0]
		double Q[16] = {0};
		for (const VPair& v : pairs) {
			const double ga = g[v.a], gb = g[v.b];
			for (int i = 0; i < 4; ++i)
				for (int j = 0; j < 4; ++j)
					Q[4 * i + j] += (ga * ga * v.A[i + j] - ga * gb * (v.C[4 * i + j] + v.C[4 * j + i]) + gb * gb * v.B[i + j]) * inv_n2;
		}
		std::vector<double> S((size_t)degree * degree), r(degree);
		for (int i = 0; i < degree; ++i) {
			for (int j = 0; j < degree; ++j) S[(size_t)i * degree + j] = Q[4 * (i + 1) + (j + 1)] + (i == j ? Mtot * inv_v2 : 0.0);
			r[i] = -Q[4 * (i + 1)];
		}
		if (!gain_cholesky_solve(S, r, degree)) OP_FAIL(OP_ERR_INVALID, "op_vignette_solve: curve system not positive definite (inconsistent statistics)");
		for (int i = 0; i < degree; ++i) a[1 + i] = r[i];
		const double e = energy();
		const bool done = !(e_prev - e > VIG_TOL * e_prev);
		e_prev = e;
		if (done) break;
	}
	// The data term fixes the gains' common scale only where the model fits; where overlaps disagree it pulls every gain
	// towards 0, and sigma_g = 1 resists weakly (misregistered overlaps: gains of 0.26).  The panorama keeps
	// its brightness: the gains are divided by their overlap-weighted mean s = sum_p N_p (g_a + g_b) / (2 sum_p N_p) --
	// ratios and curve unchanged, and s ~ 1 wherever the model fits (the prior then sets the scale to about that).
	double ssum = 0.0;
	for (const VPair& v : pairs) ssum += v.N * (g[v.a] + g[v.b]);
	const double s = ssum / (2.0 * Mtot);
	if (s > 0.0)
		for (int i = 0; i < m; ++i) g[act[i]] /= s;
	float pf[3] = {0.f, 0.f, 0.f};
	for (int i = 0; i < degree; ++i) pf[i] = (float)a[1 + i];
	const double ad[3] = {pf[0], pf[1], pf[2]};
	bool gains_ok = true;
	for (int i = 0; i < m; ++i) gains_ok = gains_ok && std::isfinite((float)g[act[i]]) && (float)g[act[i]] > 0.f;
	if (!gains_ok) OP_FAIL(OP_ERR_UNSUPPORTED, "op_vignette_solve: a fitted gain is not finite and positive: keep plain gains");
	if (!vignette_curve_positive(ad))
		OP_FAIL(OP_ERR_UNSUPPORTED, "op_vignette_solve: the fitted curve is not positive on [0, 1] (a = " + std::to_string(pf[0]) + ", " +
		        std::to_string(pf[1]) + ", " + std::to_string(pf[2]) + "): keep plain gains");
	for (int i = 0; i < m; ++i) {
		const float gv = (float)g[act[i]];
		gains[3 * act[i]] = gains[3 * act[i] + 1] = gains[3 * act[i] + 2] = gv;
	}
	for (int i = 0; i < 3; ++i) poly[i] = pf[i];
	return OP_OK;
}

}	// extern "C"
