/* vignette_overlap_ref.c -- CPU restatements of the vignetting entry points (openpano_amd/csrc/overlap.hip, blend_sample.hpp, photometric_solve.cc) for
 * tests/test_gpu_vignette.py, built like gain_block_overlap_ref.c (included below for the image type, the map and the
 * sampling rules) with -ffp-contract=off so that every fp64 / fp32 operation is the device's:
 *   vignette_overlap_ref   op_vignette_overlap (k_vignette_overlap): per pair, the count and the 30 moments of the grey
 *                          level and the radius (include/openpano_hip.h), fixed point;
 *   blend_linear_vig_ref   op_blend_vignette with the linear blender (k_blend_linear<GAIN_VIGNETTE>): every valid sample
 *                          scaled by its gains over the shared curve at its radius, both LAZY_READ branches. */
#include "gain_block_overlap_ref.c"

/* the contract's normalised squared radius and grey level, fp32 */
static float vig_rho(float r, float c, int w, int h) {
	const float fw = (float)w, fh = (float)h;
	const float dx = c - 0.5f * fw, dy = r - 0.5f * fh;
	return fminf((dx * dx + dy * dy) / (0.25f * (fw * fw + fh * fh)), 1.f);
}
static float vig_grey(const float col[3]) { return (col[0] + col[1] + col[2]) / 3.f; }

/* count: P, moments: P * 30, both zeroed by the caller */
int vignette_overlap_ref(int method, double minx, double miny, double resx, double resy, int H, int W, int n, const gref_image* imgs,
		int stride, int lazy, float clip, int64_t* count, int64_t* moments) {
	float* Y = (float*)malloc(sizeof(float) * (size_t)n);
	float* R = (float*)malloc(sizeof(float) * (size_t)n);
	int* ok = (int*)malloc(sizeof(int) * (size_t)n);
	if (!Y || !R || !ok) return -1;
	for (int i = 0; i < H; i += stride) {
		for (int j = 0; j < W; j += stride) {
			double hx, hy, hz;
			map_point(method, minx, miny, resx, resy, i, j, &hx, &hy, &hz);
			for (int k = 0; k < n; ++k) {
				float r, c, col[3];
				ok[k] = sample_rc(&imgs[k], i, j, hx, hy, hz, lazy, &r, &c, col);
				if (ok[k] && fmaxf(col[0], fmaxf(col[1], col[2])) > clip) ok[k] = 0;
				Y[k] = ok[k] ? vig_grey(col) : 0.f;
				R[k] = ok[k] ? vig_rho(r, c, imgs[k].w, imgs[k].h) : 0.f;
			}
			for (int a = 0; a < n; ++a) {
				if (!ok[a]) continue;
				for (int b = a + 1; b < n; ++b) {
					if (!ok[b]) continue;
					const long long p = (long long)a * n - (long long)a * (a + 1) / 2 + (b - a - 1);
					const double Ya = (double)Y[a], Yb = (double)Y[b], Ra = (double)R[a], Rb = (double)R[b];
					const double aa = Ya * Ya, bb = Yb * Yb, ab = Ya * Yb;
					double pa[7], pb[7];
					pa[0] = 1.0; pb[0] = 1.0;
					for (int k = 1; k < 7; ++k) { pa[k] = pa[k - 1] * Ra; pb[k] = pb[k - 1] * Rb; }
					int64_t* m = moments + 30 * p;
					count[p] += 1;
					for (int k = 0; k < 7; ++k) {
						m[k] += llrint((aa * pb[k]) * 4294967296.0);
						m[7 + k] += llrint((bb * pa[k]) * 4294967296.0);
					}
					for (int u = 0; u < 4; ++u)
						for (int v = 0; v < 4; ++v) m[14 + 4 * u + v] += llrint(((ab * pa[u]) * pb[v]) * 4294967296.0);
				}
			}
		}
	}
	free(Y); free(R); free(ok);
	return 0;
}

/* LinearBlender::run (blender.cc:24-96) with gains over the shared curve: out H x W x 3; gains n x 3; poly a1, a2, a3 */
int blend_linear_vig_ref(int method, double minx, double miny, double resx, double resy, int H, int W, int n, const gref_image* imgs,
		int lazy, int ordered_input, const float* gains, const float* poly, float* out) {
	for (int i = 0; i < H; ++i) {
		for (int j = 0; j < W; ++j) {
			double hx, hy, hz;
			map_point(method, minx, miny, resx, resy, i, j, &hx, &hy, &hz);
			float s0 = 0.f, s1 = 0.f, s2 = 0.f, wsum = 0.f;
			for (int k = 0; k < n; ++k) {
				const gref_image* im = &imgs[k];
				float r, c, col[3];
				if (!sample_rc(im, i, j, hx, hy, hz, lazy, &r, &c, col)) continue;
				const float rho = vig_rho(r, c, im->w, im->h);
				const float V = 1.f + rho * (poly[0] + rho * (poly[1] + rho * poly[2]));
				for (int ch = 0; ch < 3; ++ch) {
					const float f = gains[3 * k + ch] / V;
					if (f != 1.f) col[ch] = fminf(col[ch] * f, 1.f);
				}
				float w = (float)(0.5 - fabs((double)(c / (float)im->w) - 0.5));
				if (!ordered_input) w = (float)((double)w * (0.5 - fabs((double)(r / (float)im->h) - 0.5)));
				s0 += col[0] * w; s1 += col[1] * w; s2 += col[2] * w;
				wsum += w;
			}
			float* row = out + ((size_t)i * W + j) * 3;
			if (lazy) {
				if (wsum != 0.f) { row[0] = s0 / wsum; row[1] = s1 / wsum; row[2] = s2 / wsum; }
				else { row[0] = -1.f; row[1] = -1.f; row[2] = -1.f; }
			} else {
				if (wsum > 0) {
					const float inv = (float)(1.0 / (double)wsum);
					row[0] = s0 * inv; row[1] = s1 * inv; row[2] = s2 * inv;
				} else { row[0] = -1.f; row[1] = -1.f; row[2] = -1.f; }
			}
		}
	}
	return 0;
}
