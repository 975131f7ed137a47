/* gain_overlap_ref.c -- CPU restatement of op_gain_overlap (openpano_amd/csrc/overlap.hip: k_gain_overlap) for
 * tests/test_gpu_gain.py.  Plain C, built by the test with -ffp-contract=off so that every fp64 / fp32 operation is the
 * device's: the canvas -> image map of ConnectedImages::blend with the per-column sin / cos and per-row tan from this
 * host's libm (what the library tabulates), the linear blender's validity rules, interpolate(), and the fixed-point
 * sums llrint(col * 2^32) in int64.  Pairs (a < b) at a*n - a*(a+1)/2 + (b - a - 1). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
	const float* data;
	int h, w, mh, mw;
	double hinv[9];
	int x0, y0, x1, y1;        /* ROI on the canvas, inclusive */
} gref_image;

static int interp(const float* img, int rows, int cols, float r, float c, float out[3]) {
	const int fr = (int)floorf(r), fc = (int)floorf(c);
	if (fr < 0 || fc < 0 || fc + 1 >= cols || fr + 1 >= rows) return 0;
	r -= (float)fr; c -= (float)fc;
	const float* p00 = img + ((long long)fr * cols + fc) * 3;
	const float* p10 = p00 + (long long)cols * 3;
	if (p00[0] < 0 || p10[0] < 0 || p10[3] < 0 || p00[3] < 0) return 0;
	float w = (1 - r) * (1 - c);
	float r0 = 0.f + p00[0] * w, r1 = 0.f + p00[1] * w, r2 = 0.f + p00[2] * w;
	w = r * (1 - c);
	r0 += p10[0] * w; r1 += p10[1] * w; r2 += p10[2] * w;
	w = r * c;
	r0 += p10[3] * w; r1 += p10[4] * w; r2 += p10[5] * w;
	w = (1 - r) * c;
	r0 += p00[3] * w; r1 += p00[4] * w; r2 += p00[5] * w;
	out[0] = r0; out[1] = r1; out[2] = r2;
	return 1;
}

/* one image's sample at canvas pixel (i, j) by the linear blender's rules; 0 = none */
static int sample(const gref_image* im, int i, int j, double hx, double hy, double hz, int lazy, float col[3]) {
	const int in = lazy ? (i >= im->y0 && i < im->y1 && j >= im->x0 && j < im->x1)
	                    : (i >= im->y0 && i <= im->y1 && j >= im->x0 && j <= im->x1);
	if (!in) return 0;
	const double* d = im->hinv;
	const double rx = d[0] * hx + d[1] * hy + d[2] * hz;
	const double ry = d[3] * hx + d[4] * hy + d[5] * hz;
	const double rz = d[6] * hx + d[7] * hy + d[8] * hz;
	double ox, oy;
	if (rz < 0) { ox = -10; oy = -10; }
	else {
		const double denom = 1.0 / rz;
		ox = rx * denom + im->w * 0.5;
		oy = ry * denom + im->h * 0.5;
	}
	if (ox < 0 || ox >= im->w || oy < 0 || oy >= im->h) return 0;
	if (!interp(im->data, im->mh, im->mw, (float)oy, (float)ox, col)) return 0;
	return !(col[0] < 0);
}

/* count: n(n-1)/2, sums: n(n-1)/2 x 6, both zeroed by the caller */
int gain_overlap_ref(int method, double minx, double miny, double resx, double resy, int H, int W, int n, const gref_image* imgs,
		int stride, int lazy, int64_t* count, int64_t* sums) {
	float* col = (float*)malloc(sizeof(float) * 3 * (size_t)n);
	int* ok = (int*)malloc(sizeof(int) * (size_t)n);
	if (!col || !ok) return -1;
	for (int i = 0; i < H; i += stride) {
		for (int j = 0; j < W; j += stride) {
			double hx, hy, hz;
			if (method == 0) { hx = (double)j * resx + minx; hy = (double)i * resy + miny; hz = 1.0; }
			else {
				const double x = (double)j * resx + minx, y = (double)i * resy + miny;
				hx = sin(x); hz = cos(x); hy = method == 2 ? tan(y) : y;
			}
			for (int k = 0; k < n; ++k) ok[k] = sample(&imgs[k], i, j, hx, hy, hz, lazy, col + 3 * k);
			for (int a = 0; a < n; ++a) {
				if (!ok[a]) continue;
				for (int b = a + 1; b < n; ++b) {
					if (!ok[b]) continue;
					const long long p = (long long)a * n - (long long)a * (a + 1) / 2 + (b - a - 1);
					count[p] += 1;
					for (int c = 0; c < 3; ++c) {
						sums[6 * p + c] += llrint((double)col[3 * a + c] * 4294967296.0);
						sums[6 * p + 3 + c] += llrint((double)col[3 * b + c] * 4294967296.0);
					}
				}
			}
		}
	}
	free(col); free(ok);
	return 0;
}
