// blend_sample.hpp -- the device sampler of the blend stage: the canvas -> image map, the bilinear taps, the tile cover walk,
// one sample of the linear blender and the gain / block-gain / vignette appliers.  Shared by the blend kernels (blend.hip),
// the overlap statistics (overlap.hip) and the cylinder warp (canvas.hip); every function is inlined into its kernel.
#pragma once
#include "internal.hpp"
#include "blend_shared.hpp"

struct BlendImg {
	const void* data; int h, w;    // ImageRef::height()/width(): bounds, weights, centre.  data: fp32, or bytes when u8 is set
	int mh, mw;                    // rows / cols of the pixel buffer (differ after a cylinder pre-warp, see op_blend_image)
	int x0, y0, x1, y1;        // ROI on the canvas, inclusive (BlenderBase::Range, blender.hh:19-27)
	double hinv[9];
	long long roi_off;         // multiband: offset (pixels) of this image's ROI planes
	int rw, rh;
	int u8;                    // OP_SRC_U8: data holds mh x mw x 3 decoder bytes (read only by the U8 instances of the kernels)
};

struct BlendGeom { int method; double minx, miny, resx, resy; };

// stitch/projection.hh:29-31,38-40,66-68 for canvas pixel (i, j).  Flat: the coordinates themselves.  Cylindrical /
// spherical: colsc[j] = (sin, cos) of the column's x, rowt[i] = y (cylindrical) or tan(y) (spherical), from the host
// libm (trig_tables below); the tables have one entry past the canvas (the multiband first level visits it).
struct BlendTrig { const double2* colsc; const double* rowt; int w1, h1; };
__device__ __forceinline__ void proj2homo(const BlendGeom& g, const BlendTrig& t, int i, int j, double& hx, double& hy, double& hz) {
	if (g.method == 0) { hx = (double)j * g.resx + g.minx; hy = (double)i * g.resy + g.miny; hz = 1.0; }
	else {
		const double2 sc = t.colsc[j < t.w1 ? j : t.w1 - 1];
		hx = sc.x; hz = sc.y; hy = t.rowt[i < t.h1 ? i : t.h1 - 1];
	}
}

// the lambda of ConnectedImages::blend (stitcher_image.cc:143-151) after proj2homo
__device__ __forceinline__ void space_to_image(const BlendImg& im, double hx, double hy, double hz, double& ox, double& oy) {
	const double* d = im.hinv;
	const double rx = d[0] * hx + d[1] * hy + d[2] * hz;
	const double ry = d[3] * hx + d[4] * hy + d[5] * hz;
	const double rz = d[6] * hx + d[7] * hy + d[8] * hz;
	if (rz < 0) { ox = -10; oy = -10; return; }
	const double denom = 1.0 / rz;
	ox = rx * denom + im.w * 0.5;
	oy = ry * denom + im.h * 0.5;
}

// interpolate()'s bounds, fr < 0 || fc < 0 || fc + 1 >= cols || fr + 1 >= rows with fr = floor(r), fc = floor(c), tested on the
// floats: the same answer for every coordinate an int holds, and "outside" for the rest.  The multiband first level passes
// coordinates it has not bounded: a canvas pixel 90 degrees off a view's axis (any panorama wider than half a turn has them
// inside the ROI of a view that straddles the seam) maps to |coordinate| > 2^31, whose conversion saturates, fr + 1 wraps
// and the int test lets the taps through -- a read far outside the image.
__device__ __forceinline__ bool in_taps(int rows, int cols, float r, float c) {
	return r >= 0.f && c >= 0.f && r < (float)(rows - 1) && c < (float)(cols - 1);
}

// interpolate (lib/imgproc.cc:135-156); false = Color::NO
__device__ __forceinline__ bool interpolate(const float* __restrict__ img, int rows, int cols, float r, float c, float (&out)[3]) {
	if (!in_taps(rows, cols, r, c)) return false;
	const int fr = (int)floorf(r), fc = (int)floorf(c);
	r -= (float)fr; c -= (float)fc;
	const float* p00 = img + ((long long)fr * cols + fc) * 3;
	const float* p10 = p00 + (long long)cols * 3;
	float a0 = p00[0], a1 = p00[1], a2 = p00[2];
	if (a0 < 0) return false;
	float b0 = p10[0], b1 = p10[1], b2 = p10[2];
	if (b0 < 0) return false;
	float c0 = p10[3], c1 = p10[4], c2 = p10[5];
	if (c0 < 0) return false;
	float d0 = p00[3], d1 = p00[4], d2 = p00[5];
	if (d0 < 0) return false;
	float w = (1 - r) * (1 - c);
	float r0 = 0.f + a0 * w, r1 = 0.f + a1 * w, r2 = 0.f + a2 * w;
	w = r * (1 - c);
	r0 += b0 * w; r1 += b1 * w; r2 += b2 * w;
	w = r * c;
	r0 += c0 * w; r1 += c1 * w; r2 += c2 * w;
	w = (1 - r) * c;
	r0 += d0 * w; r1 += d1 * w; r2 += d2 * w;
	out[0] = r0; out[1] = r1; out[2] = r2;
	return true;
}

// A decoder byte as a source pixel: read_img's (float)((double)b / 255.0) (lib/imgio.cc:55-57,78-80).  Evaluated as
// (float)((double)b * (1.0 / 255.0)) -- three instructions, no table to set up, and equal to the division for all 256
// bytes (tests/test_views_cpu.py); (float)b * (1.f / 255.f) is not (126 of 256 differ).
__device__ __forceinline__ float byte_pixel(unsigned b) { return (float)((double)b * (1.0 / 255.0)); }

// interpolate() for an image of decoder bytes (OP_SRC_U8): the four taps are converted as read_img would have, then the
// fp32 sequence above, unchanged.  A byte image holds no Color::NO, so the four `< 0` tests fall away.  The footprint is two
// runs of 6 bytes at byte offset 3 (fr cols + fc) -- any alignment mod 4 -- read with byte loads: nothing outside
// [img, img + 3 rows cols) is touched, whatever the alignment of a caller-owned pointer.  (Aligned dword loads +
// v_alignbyte with the image's first and last dwords guarded measured 8 % slower: DESIGN section 12.)
__device__ __forceinline__ bool interpolate_u8(const unsigned char* __restrict__ img, int rows, int cols, float r, float c, float (&out)[3]) {
	if (!in_taps(rows, cols, r, c)) return false;
	const int fr = (int)floorf(r), fc = (int)floorf(c);
	r -= (float)fr; c -= (float)fc;
	const unsigned char* p00 = img + ((long long)fr * cols + fc) * 3;
	const unsigned char* p10 = p00 + (long long)cols * 3;
	unsigned t[12];
#pragma unroll
	for (int q = 0; q < 6; ++q) { t[q] = p00[q]; t[6 + q] = p10[q]; }
	const float a0 = byte_pixel(t[0]), a1 = byte_pixel(t[1]), a2 = byte_pixel(t[2]);
	const float d0 = byte_pixel(t[3]), d1 = byte_pixel(t[4]), d2 = byte_pixel(t[5]);
	const float b0 = byte_pixel(t[6]), b1 = byte_pixel(t[7]), b2 = byte_pixel(t[8]);
	const float c0 = byte_pixel(t[9]), c1 = byte_pixel(t[10]), c2 = byte_pixel(t[11]);
	float w = (1 - r) * (1 - c);
	float r0 = 0.f + a0 * w, r1 = 0.f + a1 * w, r2 = 0.f + a2 * w;
	w = r * (1 - c);
	r0 += b0 * w; r1 += b1 * w; r2 += b2 * w;
	w = r * c;
	r0 += c0 * w; r1 += c1 * w; r2 += c2 * w;
	w = (1 - r) * c;
	r0 += d0 * w; r1 += d1 * w; r2 += d2 * w;
	out[0] = r0; out[1] = r1; out[2] = r2;
	return true;
}

__device__ __forceinline__ bool source_interpolate(const float* img, int rows, int cols, float r, float c, float (&out)[3]) { return interpolate(img, rows, cols, r, c, out); }
__device__ __forceinline__ bool source_interpolate(const unsigned char* img, int rows, int cols, float r, float c, float (&out)[3]) { return interpolate_u8(img, rows, cols, r, c, out); }

// The one place the blend kernels read a source image.  U8: the instance of a call whose set holds a byte view -- the
// type is per image, and the walk over covering images is wave-uniform, so the branch is too; an all-fp32 call runs the
// instance without it.
template <bool U8>
__device__ __forceinline__ bool sample_source(const BlendImg& im, float r, float c, float (&out)[3]) {
	if (U8 && im.u8) return interpolate_u8((const unsigned char*)im.data, im.mh, im.mw, r, c, out);
	return interpolate((const float*)im.data, im.mh, im.mw, r, c, out);
}

// The canvas-pixel kernels below walk "every image whose ROI holds this pixel, in index order".  Testing all n ROIs per
// pixel made them scalar-bound (38 images: 38 descriptor loads and 152 compares per pixel for the two or three that
// cover it): a workgroup -- a 64 x 4 pixel tile -- first marks the images whose ROI meets its TILE (one image per lane,
// one ballot per 64 images), then every pixel walks only those, with the exact per-pixel test of the reference.
constexpr int COVER_WORDS = 64;          // images per round of the walk: 64 x 64
__device__ __forceinline__ void tile_cover(const BlendImg* __restrict__ imgs, int k0, int n, int i0, int j0, int excl, unsigned long long* s_cover) {
	const int k1 = n - k0 < COVER_WORDS * 64 ? n : k0 + COVER_WORDS * 64;
	__syncthreads();                                    // the previous round's list is no longer read
	for (int k = k0 + (int)threadIdx.x; k < ((k1 - k0 + 63) & ~63) + k0; k += 256) {
		bool hit = false;
		if (k < k1) {
			const BlendImg& im = imgs[k];
			hit = im.x0 <= j0 + 63 && im.x1 - excl >= j0 && im.y0 <= i0 + 3 && im.y1 - excl >= i0;
		}
		const unsigned long long b = __ballot(hit);
		if ((threadIdx.x & 63) == 0) s_cover[(k - k0) >> 6] = b;
	}
	__syncthreads();
}
// visit(k) for every marked image of the round starting at k0, ascending; the list is wave-uniform (scalar loop control)
template <typename F>
__device__ __forceinline__ void walk_cover(const unsigned long long* s_cover, int k0, int n, F&& visit) {
	const int words = ((n - k0 < COVER_WORDS * 64 ? n - k0 : COVER_WORDS * 64) + 63) >> 6;
	for (int wd = 0; wd < words; ++wd) {
		const unsigned long long mw = s_cover[wd];
		unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mw), hi = __builtin_amdgcn_readfirstlane((unsigned)(mw >> 32));
		while (lo) { const int b = __builtin_ctz(lo); lo &= lo - 1; visit(k0 + wd * 64 + b); }
		while (hi) { const int b = __builtin_ctz(hi); hi &= hi - 1; visit(k0 + wd * 64 + 32 + b); }
	}
}

// One sample of LinearBlender::run (blender.cc:26-36, GET_COLOR_AND_W without the weight) at canvas pixel (i, j):
// the ROI test of the branch (non-lazy: Range::contain, inclusive, blender.cc:84; lazy: the loops exclude max,
// blender.cc:49-51), ImageToAdd::map_coor (blender.hh:39-44), interpolate() != NO and col[0] >= 0.  false = the image
// adds nothing here.  r / c: the sample's image coordinates (the blend weight's operands).
template <bool U8>
__device__ __forceinline__ bool linear_sample(const BlendImg& im, int i, int j, double hx, double hy, double hz, int lazy,
		float& r, float& c, float (&col)[3]) {
	const bool in = lazy ? (i >= im.y0 && i < im.y1 && j >= im.x0 && j < im.x1)
	                     : (i >= im.y0 && i <= im.y1 && j >= im.x0 && j <= im.x1);
	if (!in) return false;
	double ox, oy;
	space_to_image(im, hx, hy, hz, ox, oy);
	if (ox < 0 || ox >= im.w || oy < 0 || oy >= im.h) return false;
	r = (float)oy; c = (float)ox;
	if (!sample_source<U8>(im, r, c, col)) return false;
	return !(col[0] < 0);
}

// Exposure gain of a valid sample (op_blend_gains): col * g clamped to 1, so a gained colour stays in [0, 1] (Color::NO,
// multiband's final clamp and write_rgb's truncation keep their meaning).  A channel whose gain is exactly 1 is left
// untouched: bilinear weights can sum one ulp above 1, and a clamp there would move the pixel off op_blend's.
__device__ __forceinline__ void apply_gain(const float* __restrict__ g, float (&col)[3]) {
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) { const float gc = g[ch]; if (gc != 1.f) col[ch] = fminf(col[ch] * gc, 1.f); }
}

// Block gains (op_gain_block_overlap / op_blend_block_gains): image k -- ImageRef size w x h, the bounds linear_sample tests
// against -- is split into bx x by blocks; block (u, v) is unit q = v * bx + u.  A sample at image coordinates (r, c) -- the
// floats linear_sample returns and interpolate() reads -- lies in the block below.  This exact fp32 expression is part of the
// contract (include/openpano_hip.h); the CPU restatements copy it.
constexpr int GAIN_NONE = 0, GAIN_IMAGE = 1, GAIN_BLOCK = 2;   // gain modes of the blend kernels
__device__ __forceinline__ int gain_block_of(float r, float c, int w, int h, int bx, int by) {
	int u = (int)floorf(c * (float)bx / (float)w), v = (int)floorf(r * (float)by / (float)h);
	u = u < 0 ? 0 : (u > bx - 1 ? bx - 1 : u);
	v = v < 0 ? 0 : (v > by - 1 ? by - 1 : v);
	return v * bx + u;
}
// one axis of the bilinear interpolation between block centres, clamped at the border: the cells i0, i1 and the weight t
__device__ __forceinline__ void gain_block_axis(float x, int nb, int dim, int& i0, int& i1, float& t) {
	const float f = x * (float)nb / (float)dim - 0.5f;
	int a = (int)floorf(f);
	a = a < 0 ? 0 : (a > nb - 1 ? nb - 1 : a);
	i0 = a; i1 = a + 1 < nb ? a + 1 : nb - 1;
	float tt = f - (float)a;
	t = tt < 0.f ? 0.f : (tt > 1.f ? 1.f : tt);
}
// The gain at (r, c) of an image whose by x bx x 3 block gains start at G, interpolated bilinearly between block centres as
// lerp(a, b, t) = a + t (b - a): a uniform map gives exactly its value (b - a = 0), so it reproduces apply_gain bit for bit.
// Then applied per channel as apply_gain does.
__device__ __forceinline__ void apply_block_gain(const float* __restrict__ G, int bx, int by, int w, int h, float r, float c, float (&col)[3]) {
	int u0, u1, v0, v1; float tx, ty;
	gain_block_axis(c, bx, w, u0, u1, tx);
	gain_block_axis(r, by, h, v0, v1, ty);
	const float* g00 = G + (v0 * bx + u0) * 3; const float* g01 = G + (v0 * bx + u1) * 3;
	const float* g10 = G + (v1 * bx + u0) * 3; const float* g11 = G + (v1 * bx + u1) * 3;
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		const float top = g00[ch] + tx * (g01[ch] - g00[ch]);
		const float bot = g10[ch] + tx * (g11[ch] - g10[ch]);
		const float gc = top + ty * (bot - top);
		if (gc != 1.f) col[ch] = fminf(col[ch] * gc, 1.f);
	}
}

// Radial vignetting shared by all views (op_vignette_overlap / op_blend_vignette): the normalised squared radius of a sample
// at image coordinates (r, c) of an image of ImageRef size w x h about the map's centre (0.5 w, 0.5 h) -- isotropic in
// pixels, 1 at the corners, clamped to [0, 1] against rounding -- and the grey level the model observes.  Both exact fp32
// expressions are part of the contract (include/openpano_hip.h); the CPU restatements copy them.
constexpr int GAIN_VIGNETTE = 3;
__device__ __forceinline__ float vignette_rho(float r, float c, int w, int h) {
	const float fw = (float)w, fh = (float)h;
	const float dx = c - 0.5f * fw, dy = r - 0.5f * fh;
	return fminf((dx * dx + dy * dy) / (0.25f * (fw * fw + fh * fh)), 1.f);
}
__device__ __forceinline__ float vignette_grey(const float (&col)[3]) { return (col[0] + col[1] + col[2]) / 3.f; }
// The gains g (3 floats) divided by the curve V = 1 + rho (a1 + rho (a2 + rho a3)) at the sample (poly = a1, a2, a3), then
// applied per channel as apply_gain does: a = 0 gives V = 1 exactly, so it reproduces apply_gain bit for bit.
__device__ __forceinline__ void apply_vignette(const float* __restrict__ g, const float* __restrict__ poly, int w, int h, float r, float c,
		float (&col)[3]) {
	const float rho = vignette_rho(r, c, w, h);
	const float V = 1.f + rho * (poly[0] + rho * (poly[1] + rho * poly[2]));
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) { const float f = g[ch] / V; if (f != 1.f) col[ch] = fminf(col[ch] * f, 1.f); }
}
// The gain of mode GM (below) at a valid sample of image k -- ImageRef size w x h -- at image coordinates (r, c); gains: the
// device table
template <int GM>
__device__ __forceinline__ void apply_gain_mode(const float* __restrict__ gains, int k, int n, int gbx, int gby, int w, int h, float r, float c,
		float (&col)[3]) {
	if (GM == GAIN_IMAGE) apply_gain(gains + 3 * (long long)k, col);
	if (GM == GAIN_BLOCK) apply_block_gain(gains + 3 * (long long)k * gbx * gby, gbx, gby, w, h, r, c, col);
	if (GM == GAIN_VIGNETTE) apply_vignette(gains + 3 * (long long)k, gains + 3 * (long long)n, w, h, r, c, col);
}
