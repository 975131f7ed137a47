// blend.hip -- final warp + blend on the device.
//
// Replaces, for the whole bundle per launch:
//   ConnectedImages::blend            stitch/stitcher_image.cc:116-155 (inverse map per canvas pixel,
//                                     stitch/projection.hh:14-71, Homography::trans homography.hh:53-58)
//   LinearBlender::run                stitch/blender.cc:24-96 (both LAZY_READ branches)
//   MultiBandBlender::run             stitch/multiband.cc:19-151 (+ GaussianBlur::blur<WeightedPixel>,
//                                     feature/gaussian.hh:30-91)
//   interpolate                       lib/imgproc.cc:135-156
//   CylinderProject::project          stitch/warp.cc:25-44
// and keeps on the host, in fp64 with the host libm exactly like the reference, the O(n)
// geometry: calc_inverse_homo / update_proj_range / get_final_resolution
// (stitcher_image.cc:36-114) and the bounds of CylinderProject::project(Shape2D&) (warp.cc:46-67).
//
// The blender API of the reference takes the coordinate map as an opaque std::function
// (blender.hh:52-56), which a device cannot call; the seam is therefore one level up, at
// ConnectedImages::blend, and the map is passed as PODs (projection method, proj_range.min,
// resolution, homo_inv per image).
//
// Numerics: coordinates in fp64 exactly in the reference's operation order (this TU is built
// with -ffp-contract=off).  The map's transcendentals are SEPARABLE: proj2homo takes sin / cos of a value that
// depends on the canvas column only and tan of one that depends on the row only (stitcher_image.cc:144-145:
// c = Vec2D(t.x, t.y) * resolution + proj_range.min), and CylinderProject's tan / cos (warp.cc:19-23) take a
// per-column argument.  They are therefore tabulated once per canvas by the HOST libm -- W + H evaluations of the
// very functions the reference calls, instead of W x H evaluations of a device libm that can differ from glibc in
// the last ulp (rounds 1-4: masks equal up to 2e-5 of the pixels, colours within 1e-4) -- and the kernels read the
// tables: every coordinate is the reference's double, bit for bit.  Colour arithmetic is fp32 in the reference's
// order, so the canvas is bit-equal for every projection (tests assert array equality).
#include "internal.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

struct op_canvas {
	float* data = nullptr;   // device, h x w x 3
	int h = 0, w = 0;
	int device = 0;
};

namespace {

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
constexpr int GAIN_MAX_BLOCKS = 16;                           // bx, by in [1, 16]
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

// ---- LinearBlender::run (blender.cc:24-96): thread per canvas pixel, images in index order.  GM: GAIN_IMAGE -- gains
// (n x 3) scale every sample (op_blend_gains); GAIN_BLOCK -- gains (n x gby x gbx x 3) are interpolated at the sample
// (op_blend_block_gains); GAIN_VIGNETTE -- gains (n x 3, then the curve's a1..a3 at gains + 3n) are divided by the shared
// curve at the sample (op_blend_vignette); GAIN_NONE -- the kernel is op_blend's.  gbx / gby are read by GAIN_BLOCK only ----
template <int GM, bool U8>
__global__ void __launch_bounds__(256) k_blend_linear(BlendGeom g, BlendTrig trig, const BlendImg* __restrict__ imgs, int n,
		float* __restrict__ out, int H, int W, int ordered_input, int lazy, const float* __restrict__ gains, int gbx, int gby) {
	__shared__ unsigned long long s_cover[COVER_WORDS];
	const int j = blockIdx.x * 64 + (threadIdx.x & 63);
	const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
	const bool live = i < H && j < W;
	double hx, hy, hz;
	proj2homo(g, trig, i, j, hx, hy, hz);
	float s0 = 0.f, s1 = 0.f, s2 = 0.f, wsum = 0.f;
	for (int k0 = 0; k0 < n; k0 += COVER_WORDS * 64) {
		tile_cover(imgs, k0, n, blockIdx.y * 4, blockIdx.x * 64, lazy ? 1 : 0, s_cover);
		if (!live) continue;
		walk_cover(s_cover, k0, n, [&](int k) {
			const BlendImg& im = imgs[k];
			float r, c, col[3];
			if (!linear_sample<U8>(im, i, j, hx, hy, hz, lazy, r, c, col)) return;
			apply_gain_mode<GM>(gains, k, n, gbx, gby, im.w, im.h, r, c, col);
			float w = (float)(0.5 - fabs((double)(c / (float)im.w) - 0.5));
			if (!ordered_input) w = (float)((double)w * (0.5 - fabs((double)(r / (float)im.h) - 0.5)));
			s0 += col[0] * w; s1 += col[1] * w; s2 += col[2] * w;
			wsum += w;
		});
	}
	if (!live) return;
	float* row = out + ((long long)i * W + j) * 3;
	if (lazy) {
		if (wsum != 0.f) { row[0] = s0 / wsum; row[1] = s1 / wsum; row[2] = s2 / wsum; }   // blender.cc:68-70
		else { row[0] = -1.f; row[1] = -1.f; row[2] = -1.f; }
	} else {
		if (wsum > 0) {            // Vector::operator/(T p) = *this * (1.0 / p), lib/geometry.hh:123-124
			const float inv = (float)(1.0 / (double)wsum);
			row[0] = s0 * inv; row[1] = s1 * inv; row[2] = s2 * inv;
		} else { row[0] = -1.f; row[1] = -1.f; row[2] = -1.f; }
	}
}

// ---- overlap statistics (op_gain_overlap, op_gain_block_overlap, op_vignette_overlap): thread per point of the canvas
// lattice (i, j) = (ti, tj) * stride; at every point, the samples of the linear blender (linear_sample: same map, same
// validity rules, same interpolation) of every covering image, and for every pair (a < b) of valid samples the pair's
// statistic.  Sums are fixed point, llrint(x * 2^32) as int64 (exact scaling; integer addition is associative, so the sums
// do not depend on the order the hardware adds them in), reduced across the wavefront (a row of 64 lattice points), then
// 64-bit atomics.  The workgroup's cover set -- images whose ROI meets its 64 x 4 tile of lattice points -- is ONE bitmask
// over all n images (dynamic LDS, ceil(n / 64) words), so pairs may straddle any 64-image word.  It is walked in chunks of
// GAIN_CH images whose samples stay in registers (fully unrolled: constant indices, no scratch); the pairs of a chunk with
// itself, then with every later covered image, one at a time.  A tile is usually covered by <= 4 images: one chunk, every
// image sampled once.
constexpr int GAIN_CH = 8;
constexpr double GAIN_FIX = 4294967296.0;       // 2^32
constexpr int GAIN_MAX_IMAGES = 64 * 4096;       // cover bitmask: 4096 words = 32 KB of LDS
// smallest covered image index >= k (k wave-uniform), or words * 64 when there is none; wave-uniform
__device__ __forceinline__ int next_cover(const unsigned long long* s_cover, int words, int k) {
	for (int wd = k >> 6; wd < words; ++wd) {
		unsigned long long m = s_cover[wd];
		if (wd == (k >> 6)) m &= ~0ull << (k & 63);
		const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
		if (lo) return wd * 64 + __builtin_ctz(lo);
		if (hi) return wd * 64 + 32 + __builtin_ctz(hi);
	}
	return words * 64;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}
// pair (a < b) of n images (include/openpano_hip.h)
__host__ __device__ __forceinline__ long long pair_index(int a, int b, int n) { return (long long)a * n - (long long)a * (a + 1) / 2 + (b - a - 1); }

// The walk of the three statistics kernels over a statistic S.  A slot -- one image's sample at this lattice point -- has
// two parts, of types S::P1 and S::P2, and the chunk keeps each part in its own plain array (an array of slot structs, or a
// struct of the arrays, leaves the chunk in scratch memory).  S::clear(p1, p2): the slot without a sample.  S::sample(p1, p2,
// im, lin): the slot of image im, where lin(im, r, c, col) is linear_sample at this lattice point; false: no valid sample,
// or one the statistic refuses.  S::pair(a, b, n, va, p1a, p2a, vb, p1b, p2b): the statistic of the pair (a < b).
template <bool U8, typename S>
__device__ __forceinline__ void overlap_walk(const BlendGeom& g, const BlendTrig& trig, const BlendImg* imgs, int n,
		int H, int W, int stride, int lazy, const S& stat) {
	extern __shared__ unsigned long long s_gcover[];
	const int words = (n + 63) >> 6;
	const int i = (blockIdx.y * 4 + (threadIdx.x >> 6)) * stride;
	const int j = (blockIdx.x * 64 + (threadIdx.x & 63)) * stride;
	const bool live = i < H && j < W;
	{	// tile_cover over all n images at once; the tile spans 3 * stride rows and 63 * stride columns of the canvas
		const int i0 = blockIdx.y * 4 * stride, j0 = blockIdx.x * 64 * stride, excl = lazy ? 1 : 0;
		for (int k = (int)threadIdx.x; k < words * 64; k += 256) {
			bool hit = false;
			if (k < n) {
				const BlendImg& im = imgs[k];
				hit = im.x0 <= j0 + 63 * stride && im.x1 - excl >= j0 && im.y0 <= i0 + 3 * stride && im.y1 - excl >= i0;
			}
			const unsigned long long b = __ballot(hit);
			if ((threadIdx.x & 63) == 0) s_gcover[k >> 6] = b;
		}
		__syncthreads();
	}
	double hx, hy, hz;
	proj2homo(g, trig, i, j, hx, hy, hz);
	auto lin = [&](const BlendImg& im, float& r, float& c, float (&col)[3]) { return live && linear_sample<U8>(im, i, j, hx, hy, hz, lazy, r, c, col); };
	int a0 = next_cover(s_gcover, words, 0);
	while (a0 < n) {
		int ka[GAIN_CH]; bool va[GAIN_CH]; typename S::P1 p1a[GAIN_CH]; typename S::P2 p2a[GAIN_CH];
		int k = a0;
#pragma unroll
		for (int s = 0; s < GAIN_CH; ++s) {
			ka[s] = k;
			va[s] = false; stat.clear(p1a[s], p2a[s]);
			if (k < n) { va[s] = stat.sample(p1a[s], p2a[s], imgs[k], lin); k = next_cover(s_gcover, words, k + 1); }
		}
#pragma unroll
		for (int s = 0; s < GAIN_CH; ++s)
#pragma unroll
			for (int t = s + 1; t < GAIN_CH; ++t)
				if (ka[t] < n) stat.pair(ka[s], ka[t], n, va[s], p1a[s], p2a[s], va[t], p1a[t], p2a[t]);
		const int a1 = k;                               // first covered image after this chunk
		for (int b = a1; b < n; b = next_cover(s_gcover, words, b + 1)) {
			typename S::P1 p1b; typename S::P2 p2b;
			stat.clear(p1b, p2b);
			const bool vb = stat.sample(p1b, p2b, imgs[b], lin);
#pragma unroll
			for (int s = 0; s < GAIN_CH; ++s) stat.pair(ka[s], b, n, va[s], p1a[s], p2a[s], vb, p1b, p2b);
		}
		a0 = a1;
	}
}

// ---- exposure statistics (Brown & Lowe, IJCV 2007, section 6) for op_gain_overlap: a slot holds its sample's colour; for
// every pair (a < b) of valid samples N_ab += 1, S_ab[c] += col_a[c], S_ba[c] += col_b[c]: a pair's six sums are reduced
// across the wavefront, then one 64-bit atomic per value.  x / y: the samples of a / b, valid as linear_sample said (va / vb)
__device__ __forceinline__ void gain_pair(int a, int b, int n, bool va, const float (&x)[3], bool vb, const float (&y)[3],
		unsigned long long* __restrict__ count, unsigned long long* __restrict__ sums) {
	const bool both = va && vb;
	const unsigned long long bal = __ballot(both);
	if (!bal) return;                                   // wave-uniform
	long long v[6];
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		v[ch] = both ? llrint((double)x[ch] * GAIN_FIX) : 0;
		v[3 + ch] = both ? llrint((double)y[ch] * GAIN_FIX) : 0;
	}
#pragma unroll
	for (int q = 0; q < 6; ++q) v[q] = wave_sum(v[q]);
	if ((threadIdx.x & 63) == 0) {
		const long long p = pair_index(a, b, n);
		atomicAdd(count + p, (unsigned long long)__popcll(bal));
#pragma unroll
		for (int q = 0; q < 6; ++q) atomicAdd(sums + 6 * p + q, (unsigned long long)v[q]);
	}
}
struct NoPart {};
struct GainStat {                                       // a slot: the colour
	using P1 = float[3]; using P2 = NoPart;
	unsigned long long* count; unsigned long long* sums;
	__device__ __forceinline__ void clear(P1&, P2&) const {}
	template <typename L> __device__ __forceinline__ bool sample(P1& x, P2&, const BlendImg& im, L&& lin) const { float r, c; return lin(im, r, c, x); }
	__device__ __forceinline__ void pair(int a, int b, int n, bool va, const P1& x, const P2&, bool vb, const P1& y, const P2&) const {
		gain_pair(a, b, n, va, x, vb, y, count, sums);
	}
};
template <bool U8>
__global__ void __launch_bounds__(256) k_gain_overlap(BlendGeom g, BlendTrig trig, const BlendImg* __restrict__ imgs, int n,
		int H, int W, int stride, int lazy, unsigned long long* __restrict__ count, unsigned long long* __restrict__ sums) {
	overlap_walk<U8>(g, trig, imgs, n, H, W, stride, lazy, GainStat{count, sums});
}

// ---- block statistics for op_gain_block_overlap: k_gain_overlap with every slot also carrying its sample's block
// (gain_block_of), and the statistics of pair p split by block pair, entry e = p * B^2 + qa * B + qb (B = bx * by).  The
// lanes of a wavefront -- a row of 64 lattice points -- can fall into different block pairs where a block border crosses
// the row, so a pair is reduced per distinct key: the key of the first lane left (readlane), the butterfly sums of the
// lanes sharing it, one set of 64-bit atomics, those lanes dropped, again.  Most wavefronts hold one key: one round.
constexpr long long GAIN_BLOCK_MAX_ENTRIES = 1ll << 22;    // P * B^2 (include/openpano_hip.h)
constexpr long long GAIN_BLOCK_MAX_UNKNOWNS = 4096;        // n * B, op_gain_block_solve's dense Cholesky
__device__ __forceinline__ void gain_block_pair(int a, int b, int n, int nblk, bool va, int qa, const float (&x)[3], bool vb, int qb,
		const float (&y)[3], unsigned long long* __restrict__ count, unsigned long long* __restrict__ sums) {
	const bool both = va && vb;
	unsigned long long bal = __ballot(both);
	if (!bal) return;                                   // wave-uniform
	long long v[6];
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		v[ch] = both ? llrint((double)x[ch] * GAIN_FIX) : 0;
		v[3 + ch] = both ? llrint((double)y[ch] * GAIN_FIX) : 0;
	}
	const int key = qa * nblk + qb;
	const long long base = pair_index(a, b, n) * nblk * nblk;
	while (bal) {                                       // wave-uniform: one round per distinct block pair
		const int k0 = __builtin_amdgcn_readlane(key, __builtin_ctzll(bal));
		const bool mine = both && key == k0;
		const unsigned long long mb = __ballot(mine);
		long long s[6];
#pragma unroll
		for (int q = 0; q < 6; ++q) s[q] = wave_sum(mine ? v[q] : 0);
		if ((threadIdx.x & 63) == 0) {
			const long long e = base + k0;
			atomicAdd(count + e, (unsigned long long)__popcll(mb));
#pragma unroll
			for (int q = 0; q < 6; ++q) atomicAdd(sums + 6 * e + q, (unsigned long long)s[q]);
		}
		bal &= ~mb;
	}
}
struct GainBlockStat {                                  // a slot: the colour and its block
	using P1 = float[3]; using P2 = int;
	int bx, by; unsigned long long* count; unsigned long long* sums;
	__device__ __forceinline__ void clear(P1&, P2& q) const { q = 0; }
	template <typename L> __device__ __forceinline__ bool sample(P1& x, P2& q, const BlendImg& im, L&& lin) const {
		float r, c;
		if (!lin(im, r, c, x)) return false;
		q = gain_block_of(r, c, im.w, im.h, bx, by);
		return true;
	}
	__device__ __forceinline__ void pair(int a, int b, int n, bool va, const P1& x, P2 qa, bool vb, const P1& y, P2 qb) const {
		gain_block_pair(a, b, n, bx * by, va, qa, x, vb, qb, y, count, sums);
	}
};
template <bool U8>
__global__ void __launch_bounds__(256) k_gain_block_overlap(BlendGeom g, BlendTrig trig, const BlendImg* __restrict__ imgs, int n,
		int H, int W, int stride, int lazy, int bx, int by, unsigned long long* __restrict__ count, unsigned long long* __restrict__ sums) {
	overlap_walk<U8>(g, trig, imgs, n, H, W, stride, lazy, GainBlockStat{bx, by, count, sums});
}

// ---- vignetting statistics for op_vignette_overlap: every slot carries the grey level Y and the radius rho of its sample
// instead of its colour; a sample whose largest channel exceeds `clip` does not take part (saturated).  For every pair
// (a < b) of valid samples, with pa[k] = rho_a^k, pb[k] = rho_b^k (fp64, pa[0] = 1, pa[k] = pa[k-1] * rho_a):
//   N += 1,  A_k += (Ya Ya) pb[k],  B_k += (Yb Yb) pa[k]  (k = 0..6),  C_ij += ((Ya Yb) pa[i]) pb[j]  (i, j = 0..3),
// each product in fp64 in that order from the fp32 Y / rho, summed as llrint(x 2^32) in int64.  Every term lies in [0, 1]
// (clip <= 1, rho clamped to [0, 1]) and the host caps the lattice at 2^30 points, so no sum can overflow.  Moment m of pair
// p at moments[30 p + m]: A_k at m = k, B_k at 7 + k, C_ij at 14 + 4 i + j.  A wavefront reduces the 30 moments one at a
// time (butterfly: every lane ends with the sum) and lane m keeps moment m; lane 30 the count -- then ONE atomic instruction
// of 31 lanes per pair instead of 31 from lane 0.
constexpr int VIG_MOMENTS = 30;
constexpr long long VIG_MAX_LATTICE = 1ll << 30;           // lattice points per call: bounds every pair's sums (see above)
__device__ __forceinline__ void vignette_pair(int a, int b, int n, bool va, float ya, float ra, bool vb, float yb, float rb,
		unsigned long long* __restrict__ count, unsigned long long* __restrict__ moments) {
	const bool both = va && vb;
	const unsigned long long bal = __ballot(both);
	if (!bal) return;                                   // wave-uniform
	const int lane = threadIdx.x & 63;
	const double Ya = (double)ya, Yb = (double)yb, Ra = (double)ra, Rb = (double)rb;
	const double aa = Ya * Ya, bb = Yb * Yb, ab = Ya * Yb;
	long long mine = (long long)__popcll(bal);           // lane 30's value; lanes 0..29 replace it with their moment
	// one moment per trip, x = (base pa[i]) pb[j]: A_k = (aa 1) pb[k], B_k = (bb pa[k]) 1 -- the products stated above,
	// since multiplying by 1.0 is exact.  Kept a loop (uniform trip counts, no arrays): 28 + 8 inlined pairs per chunk.
#pragma unroll 1
	for (int m = 0; m < VIG_MOMENTS; ++m) {
		const int pi = m < 7 ? 0 : (m < 14 ? m - 7 : (m - 14) >> 2), pj = m < 7 ? m : (m < 14 ? 0 : (m - 14) & 3);
		const double base = m < 7 ? aa : (m < 14 ? bb : ab);
		double pa = 1.0, pb = 1.0;
		for (int q = 0; q < pi; ++q) pa *= Ra;
		for (int q = 0; q < pj; ++q) pb *= Rb;
		const double x = (base * pa) * pb;
		const long long s = wave_sum(both ? llrint(x * GAIN_FIX) : 0);
		if (lane == m) mine = s;
	}
	if (lane <= VIG_MOMENTS) {
		const long long p = pair_index(a, b, n);
		atomicAdd(lane < VIG_MOMENTS ? moments + (long long)VIG_MOMENTS * p + lane : count + p, (unsigned long long)mine);
	}
}
struct VignetteStat {                                   // a slot: the grey level and the radius
	using P1 = float; using P2 = float;
	float clip; unsigned long long* count; unsigned long long* moments;
	__device__ __forceinline__ void clear(P1& y, P2& rho) const { y = 0.f; rho = 0.f; }
	template <typename L> __device__ __forceinline__ bool sample(P1& y, P2& rho, const BlendImg& im, L&& lin) const {
		float r, c, col[3];
		if (!lin(im, r, c, col) || fmaxf(col[0], fmaxf(col[1], col[2])) > clip) return false;   // clip: saturated
		y = vignette_grey(col);
		rho = vignette_rho(r, c, im.w, im.h);
		return true;
	}
	__device__ __forceinline__ void pair(int a, int b, int n, bool va, P1 ya, P2 ra, bool vb, P1 yb, P2 rb) const {
		vignette_pair(a, b, n, va, ya, ra, vb, yb, rb, count, moments);
	}
};
template <bool U8>
__global__ void __launch_bounds__(256) k_vignette_overlap(BlendGeom g, BlendTrig trig, const BlendImg* __restrict__ imgs, int n,
		int H, int W, int stride, int lazy, float clip, unsigned long long* __restrict__ count, unsigned long long* __restrict__ moments) {
	overlap_walk<U8>(g, trig, imgs, n, H, W, stride, lazy, VignetteStat{clip, count, moments});
}

// ---- create_first_level + update_weight_map (multiband.cc:19-56,125-143) in ONE pass, thread per canvas pixel:
// proj2homo once per pixel (it does not depend on the image), then every image whose ROI covers the pixel in index
// order: its level-0 WeightedPixel is written with weight 0 while the winner of the winner-takes-all map -- the first
// image with the strictly largest weight, as the reference's `if (w > max)` walk finds it -- is tracked in registers;
// the winner's weight is then set to 1 with one 4-byte store.  The ROI planes are written once and never read back
// (the two-kernel form re-read every weight and rewrote it: 0.49 GB of the 1.33 GB the two kernels moved), and the
// target canvas / its "seen" mask are initialised here too (fill(target, Color::NO), multiband.cc:60-61).
// GM (as k_blend_linear's): the level-0 colours are the gained samples (op_blend_gains, op_blend_block_gains -- the block
// gain interpolated at the floats interpolate() reads; op_blend_vignette -- the curve at those floats); the weights do not
// depend on colour.
template <int GM, bool U8>
__global__ void __launch_bounds__(256) k_mb_first_fused(BlendGeom g, BlendTrig trig, const BlendImg* __restrict__ imgs, int n,
		float4* __restrict__ cur, unsigned char* __restrict__ mask, float* __restrict__ out, unsigned char* __restrict__ tmask, int H, int W,
		const float* __restrict__ gains, int gbx, int gby) {
	const int j = blockIdx.x * 64 + (threadIdx.x & 63);
	const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
	// The target is as large as the largest bottom-right ROI coordinate (blender.cc:21) while ROIs are inclusive
	// (blender.hh:19-27): an ROI's last column / row can lie ONE pixel outside the target.  The reference still builds
	// that pixel of the image's level 0 (it feeds the blurs) but its weight-map walk never visits it, so it keeps its
	// own weight; the grid therefore covers (H + 1) x (W + 1) and only pixels inside the target take part in the map.
	__shared__ unsigned long long s_cover[COVER_WORDS];
	const bool live = !(i > H || j > W);
	const bool inside = i < H && j < W;
	double hx, hy, hz;
	proj2homo(g, trig, i, j, hx, hy, hz);
	float mx = 0.f; long long maxe = -1;
	for (int k0 = 0; k0 < n; k0 += COVER_WORDS * 64) {
		tile_cover(imgs, k0, n, blockIdx.y * 4, blockIdx.x * 64, 0, s_cover);
		if (!live) continue;
		walk_cover(s_cover, k0, n, [&](int k) {
			const BlendImg& im = imgs[k];
			if (!(i >= im.y0 && i <= im.y1 && j >= im.x0 && j <= im.x1)) return;
			const long long e = im.roi_off + (long long)(i - im.y0) * im.rw + (j - im.x0);
			double ox, oy;
			space_to_image(im, hx, hy, hz, ox, oy);
			float col[3];
			bool ok = sample_source<U8>(im, (float)oy, (float)ox, col);
			if (ok) { float mn = fminf(col[0], fminf(col[1], col[2])); if (mn < 0) ok = false; }
			if (ok) apply_gain_mode<GM>(gains, k, n, gbx, gby, im.w, im.h, (float)oy, (float)ox, col);
			float4 px = make_float4(0.f, 0.f, 0.f, 0.f);
			if (ok) {
				const double x = ox / (double)im.w - 0.5, y = oy / (double)im.h - 0.5;
				const double v = (0.5 - fabs(x)) * (0.5 - fabs(y));
				const float w = (float)((v > 0.0 ? v : 0.0) + 1e-6);
				px = make_float4(col[0], col[1], col[2], inside ? 0.f : w);
				if (w > mx) { mx = w; maxe = e; }                     // multiband.cc:133-137
			}
			cur[e] = px;
			mask[e] = ok ? 0 : 1;
		});
	}
	if (!inside) return;
	if (maxe >= 0) ((float*)&cur[maxe])[3] = 1.f;
	const long long pe = (long long)i * W + j;
	out[pe * 3] = -1.f; out[pe * 3 + 1] = -1.f; out[pe * 3 + 2] = -1.f;
	tmask[pe] = 0;
}

// ---- GaussianBlur::blur<WeightedPixel> (feature/gaussian.hh:30-91): column pass then row pass,
// replicate borders, sequential fp32 multiply-add in tap order on all 4 channels ----
struct BlurTaps { int center; float k[2 * OP_MAX_KCENTER + 1]; };

// CT > 0: half-width known at compile time (6 and 9 for the shipped window factor): the taps are
// unrolled and all loads of a pixel are in flight together; CT == 0: any half-width.
template <bool COLS, int CT>
__global__ void __launch_bounds__(256) k_mb_blur(const BlendImg* __restrict__ imgs, BlurTaps taps,
		const float4* __restrict__ src, float4* __restrict__ dst) {
	const BlendImg& im = imgs[blockIdx.y];
	const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
	if (e >= (long long)im.rw * im.rh) return;
	const int i = (int)(e / im.rw), j = (int)(e % im.rw);
	const float4* base = src + im.roi_off;
	float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
	if (CT > 0) {
		float4 v[2 * (CT > 0 ? CT : 1) + 1];
#pragma unroll
		for (int k = -CT; k <= CT; ++k) {
			if (COLS) { int ii = i + k; ii = ii < 0 ? 0 : (ii > im.rh - 1 ? im.rh - 1 : ii); v[k + CT] = base[(long long)ii * im.rw + j]; }
			else { int jj = j + k; jj = jj < 0 ? 0 : (jj > im.rw - 1 ? im.rw - 1 : jj); v[k + CT] = base[(long long)i * im.rw + jj]; }
		}
#pragma unroll
		for (int k = 0; k <= 2 * CT; ++k) {
			const float kv = taps.k[k];
			t.w += v[k].w * kv; t.x += v[k].x * kv; t.y += v[k].y * kv; t.z += v[k].z * kv;
		}
	} else {
		const int C = taps.center;
		for (int k = -C; k <= C; ++k) {
			float4 v;
			if (COLS) { int ii = i + k; ii = ii < 0 ? 0 : (ii > im.rh - 1 ? im.rh - 1 : ii); v = base[(long long)ii * im.rw + j]; }
			else { int jj = j + k; jj = jj < 0 ? 0 : (jj > im.rw - 1 ? im.rw - 1 : jj); v = base[(long long)i * im.rw + jj]; }
			const float kv = taps.k[k + C];
			t.w += v.w * kv; t.x += v.x * kv; t.y += v.y * kv; t.z += v.z * kv;
		}
	}
	dst[im.roi_off + e] = t;
}

// ---- the same blur, both passes in ONE kernel (the shipped window factor: half-widths 6 and 9).
// The two-pass form above moves every WeightedPixel plane through HBM twice per level and re-reads each
// source pixel 2C+1 times from cache (measured: 1.23 GB of traffic per launch for 0.44 GB algorithmic).
// Here a workgroup owns a band of 256 - 2C output columns and walks down a segment of rows:
//   column pass  thread = column (band + C halo columns either side, clamped = replicate border); the
//                2C+1 source rows around the current row live in registers as a rotating window (one
//                coalesced 16-byte load per thread and row), the reference's  tmp += line[i+k]*kernel[k]
//                runs in tap order on all four channels;
//   row pass     the column-pass row goes to LDS (double buffered: one barrier per row), thread = output
//                column reads its 2C+1 neighbours as b128 and applies the same taps in order.
// The intermediate plane never reaches HBM; a source pixel is read once per band (+ the segment halo).
// FIRST (level 0 -> 1): the band of level 0 (multiband.cc:75-110) is written here as well.  After the
// winner-takes-all map exactly one image has weight 1 at a target pixel and every other one 0, so the reference's
// sum over images has a single term, (cur - next) * 1 / 1: the winner's thread holds cur (its column window) and next
// (just computed) and stores the band into the untouched target -- the level-0 pass of k_mb_accumulate (a read of
// every image's ROI plane) disappears.
// Waits (round 5).  vmcnt counts loads AND stores, in issue order, and __syncthreads() carries a workgroup fence that waits
// for every store in flight: the first form of this kernel -- store row r, load row r + CT + 1, __syncthreads() -- waited
// for the acknowledgement of the row it had just written, once per row.  Now (i) the barrier is LDS-only (the rows written
// are never read back here), (ii) the source row of the NEXT iteration is requested at the top of an iteration, i.e. BEFORE
// this iteration's stores, so that its wait (one iteration later) has only those stores behind it, and (iii) every
// wavefront issues the same number of store instructions per row -- lanes that must not write get an offset beyond the
// buffer descriptor's range, which the hardware drops -- so that number is a compile-time constant and the compiler's own
// wait for the load is `vmcnt(<stores>)`: no store acknowledgement is ever waited for.  The window holds one row more
// (2 CT + 2 slots: the row in flight must not land on a row still in use), hence segments of k x (2 CT + 2) rows.
__device__ __forceinline__ void blur_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
typedef unsigned u32x4b __attribute__((ext_vector_type(4)));
template <int CT, bool FIRST>
__global__ void __launch_bounds__(256) k_mb_blur_fused(const BlendImg* __restrict__ imgs, BlurTaps taps,
		const float4* __restrict__ src, float4* __restrict__ dst, float* __restrict__ target, unsigned char* __restrict__ tmask, int H, int W) {
	constexpr int NT = 2 * CT + 1;          // taps
	constexpr int NS = NT + 1;              // window slots
	constexpr int TWO = 256 - 2 * CT;       // output columns of a band
	constexpr int SEG = (CT <= 6 ? 8 : 6) * NS;   // rows of a segment (a whole number of window rotations; its 2 CT halo rows are re-read)
	__shared__ float4 s_mid[2][256];
	const BlendImg& im = imgs[blockIdx.y];
	const int rw = im.rw, rh = im.rh;
	const int nbands = (rw + TWO - 1) / TWO, nsegs = (rh + SEG - 1) / SEG;
	if ((int)blockIdx.x >= nbands * nsegs) return;
	const int band = blockIdx.x % nbands, seg = blockIdx.x / nbands;
	const int t = threadIdx.x;
	const int x = band * TWO - CT + t;                        // this thread's column (may lie in the halo / outside)
	const int xc = x < 0 ? 0 : (x > rw - 1 ? rw - 1 : x);      // replicate border
	const int r0 = seg * SEG, r1 = r0 + SEG < rh ? r0 + SEG : rh;
	const float4* base = src + im.roi_off;
	float4* out = dst + im.roi_off;
	const bool writer = t >= CT && t < 256 - CT && x < rw;     // x >= 0 for these threads
	float kk[NT];
#pragma unroll
	for (int k = 0; k < NT; ++k) kk[k] = taps.k[k];
	auto row_at = [&](int r) { const int rc = r < 0 ? 0 : (r > rh - 1 ? rh - 1 : r); return base[(long long)rc * rw + xc]; };
	float4 v[NS];                           // slot of row q is (q - (r0 - CT)) % NS
#pragma unroll
	for (int k = 0; k < NT; ++k) v[k] = row_at(r0 - CT + k);   // rows r0 - CT .. r0 + CT: the first row's whole window
	const unsigned row_bytes = (unsigned)rw * 16u;
	const unsigned xoff = writer ? (unsigned)x * 16u : 0x80000000u;       // beyond any row: dropped
	for (int rb = r0; rb < r1; rb += NS) {
#pragma unroll
		for (int u = 0; u < NS; ++u) {
			const int r = rb + u;
			// the NEXT row's last source row, requested before this row's stores; its slot held row r - CT - 1, dead since the previous row
			v[(u + NT) % NS] = row_at(r + CT + 1);
			float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
			for (int k = 0; k < NT; ++k) {                   // tap k multiplies row r - CT + k = slot (u + k) % NS
				const float4 s = v[(u + k) % NS]; const float kv = kk[k];
				c.w += s.w * kv; c.x += s.x * kv; c.y += s.y * kv; c.z += s.z * kv;
			}
			s_mid[(r - r0) & 1][t] = c;                       // double buffered: the readers of row r - 1 may still be at work
			blur_lds_barrier();
			float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
			if (writer) {
				const float4* m = &s_mid[(r - r0) & 1][t - CT];
#pragma unroll
				for (int k = 0; k < NT; ++k) {
					const float4 s = m[k]; const float kv = kk[k];
					o.w += s.w * kv; o.x += s.x * kv; o.y += s.y * kv; o.z += s.z * kv;
				}
			}
			// one 16-byte store instruction per wavefront and row, whatever its lanes do (rows past the segment: dropped as well)
			const bool live = r < r1;
			{
				const int rc = live ? r : 0;
				const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out + (long long)rc * rw, 0, live ? row_bytes : 0u, 0x00020000);
				__builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4b, o), rs, xoff, 0, 0);
			}
			if (FIRST) {
				const float4 cc = v[(u + CT) % NS];              // level-0 pixel (r, x): the centre tap's row of this thread's own column
				const int ti = im.y0 + r, tj = im.x0 + x;
				const bool win = writer && live && cc.w > 0 && ti < H && tj < W;     // the winner (weight 1); a masked pixel has weight 0
				float s0 = 0.f, s1 = 0.f, s2 = 0.f, wsum = 0.f;
				s0 += (cc.x - o.x) * cc.w; s1 += (cc.y - o.y) * cc.w; s2 += (cc.z - o.z) * cc.w; wsum += cc.w;
				s0 /= wsum; s1 /= wsum; s2 /= wsum;
				const bool rowok = live && ti < H;
				const int tic = rowok ? ti : 0;
				const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(target + (long long)tic * W * 3, 0, rowok ? (unsigned)W * 12u : 0u, 0x00020000);
				const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(tmask + (long long)tic * W, 0, rowok ? (unsigned)W : 0u, 0x00020000);
				const unsigned to = win ? (unsigned)tj * 12u : 0x80000000u, mo = win ? (unsigned)tj : 0x80000000u;
				__builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, s0), rt, to, 0, 0);
				__builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, s1), rt, to, 4, 0);
				__builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, s2), rt, to, 8, 0);
				__builtin_amdgcn_raw_buffer_store_b8((unsigned char)1, rm, mo, 0, 0);
			}
		}
	}
}

// ---- one band (multiband.cc:75-110): thread per canvas pixel; the last band also clamps (:112-121) ----
__global__ void __launch_bounds__(256) k_mb_accumulate(const BlendImg* __restrict__ imgs, int n,
		const float4* __restrict__ cur, const float4* __restrict__ nxt, const unsigned char* __restrict__ mask,
		float* __restrict__ out, unsigned char* __restrict__ tmask, int H, int W, int is_last) {
	const int j = blockIdx.x * 64 + (threadIdx.x & 63);
	const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (i >= H || j >= W) return;
	float s0 = 0.f, s1 = 0.f, s2 = 0.f, wsum = 0.f;
	for (int k = 0; k < n; ++k) {
		const BlendImg& im = imgs[k];
		if (!(i >= im.y0 && i <= im.y1 && j >= im.x0 && j <= im.x1)) continue;
		const long long e = im.roi_off + (long long)(i - im.y0) * im.rw + (j - im.x0);
		if (mask[e]) continue;
		const float4 cc = cur[e];
		if (cc.w <= 0) continue;
		if (!is_last) {
			const float4 cn = nxt[e];
			s0 += (cc.x - cn.x) * cc.w; s1 += (cc.y - cn.y) * cc.w; s2 += (cc.z - cn.z) * cc.w;
		} else {
			s0 += cc.x * cc.w; s1 += cc.y * cc.w; s2 += cc.z * cc.w;
		}
		wsum += cc.w;
	}
	const long long pe = (long long)i * W + j;
	float* p = out + pe * 3;
	bool seen = tmask[pe] != 0;
	float p0 = p[0], p1 = p[1], p2 = p[2];
	if (!((double)wsum < 1e-6)) {
		s0 /= wsum; s1 /= wsum; s2 /= wsum;
		if (!seen) { p0 = s0; p1 = s1; p2 = s2; seen = true; tmask[pe] = 1; }
		else { p0 += s0; p1 += s1; p2 += s2; }
	}
	if (is_last && seen) {
		p0 = fmaxf(fminf(p0, 1.0f), 0.f); p1 = fmaxf(fminf(p1, 1.0f), 0.f); p2 = fmaxf(fminf(p2, 1.0f), 0.f);
	}
	p[0] = p0; p[1] = p1; p[2] = p2;
}

// ---- all remaining bands in ONE pass over the canvas.  The per-level form above reads, for every canvas pixel and every
// image covering it, the level's plane AND the next one (which the next level's pass reads again as its own), and moves
// the canvas through HBM once per level.  With every level's plane kept (they are a few hundred MB), a thread walks the
// covering images once, reads each level's WeightedPixel once, keeps one (sum, weight) accumulator per level -- each
// level's sum still runs over the images in index order -- and applies the bands to its canvas pixel in level order:
// the same operations on the same operands in the same order as NL launches of k_mb_accumulate.
#define OP_MB_MAX_LEVELS 6
struct BandPlanes { const float4* lv[OP_MB_MAX_LEVELS]; };
template <int NL>          // levels P.lv[0 .. NL-1]; the last one is the final level of the pyramid (no next plane; clamps)
__global__ void __launch_bounds__(256) k_mb_bands(const BlendImg* __restrict__ imgs, int n, BandPlanes P,
		const unsigned char* __restrict__ mask, float* __restrict__ out, unsigned char* __restrict__ tmask, int H, int W) {
	const int j = blockIdx.x * 64 + (threadIdx.x & 63);
	const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
	__shared__ unsigned long long s_cover[COVER_WORDS];
	const bool live = i < H && j < W;
	float s0[NL], s1[NL], s2[NL], ws[NL];
#pragma unroll
	for (int l = 0; l < NL; ++l) { s0[l] = 0.f; s1[l] = 0.f; s2[l] = 0.f; ws[l] = 0.f; }
	for (int k0 = 0; k0 < n; k0 += COVER_WORDS * 64) {
		tile_cover(imgs, k0, n, blockIdx.y * 4, blockIdx.x * 64, 0, s_cover);
		if (!live) continue;
		walk_cover(s_cover, k0, n, [&](int k) {
			const BlendImg& im = imgs[k];
			if (!(i >= im.y0 && i <= im.y1 && j >= im.x0 && j <= im.x1)) return;
			const long long e = im.roi_off + (long long)(i - im.y0) * im.rw + (j - im.x0);
			if (mask[e]) return;
			float4 lvl[NL];
#pragma unroll
			for (int l = 0; l < NL; ++l) lvl[l] = P.lv[l][e];
#pragma unroll
			for (int l = 0; l < NL; ++l) {
				const float4 cc = lvl[l];
				if (cc.w <= 0) continue;
				if (l < NL - 1) {
					const float4 cn = lvl[l + 1];
					s0[l] += (cc.x - cn.x) * cc.w; s1[l] += (cc.y - cn.y) * cc.w; s2[l] += (cc.z - cn.z) * cc.w;
				} else {
					s0[l] += cc.x * cc.w; s1[l] += cc.y * cc.w; s2[l] += cc.z * cc.w;
				}
				ws[l] += cc.w;
			}
		});
	}
	if (!live) return;
	const long long pe = (long long)i * W + j;
	float* p = out + pe * 3;
	const bool seen0 = tmask[pe] != 0;
	bool seen = seen0;
	float p0 = p[0], p1 = p[1], p2 = p[2];
#pragma unroll
	for (int l = 0; l < NL; ++l) {
		if (!((double)ws[l] < 1e-6)) {
			const float a0 = s0[l] / ws[l], a1 = s1[l] / ws[l], a2 = s2[l] / ws[l];
			if (!seen) { p0 = a0; p1 = a1; p2 = a2; seen = true; }
			else { p0 += a0; p1 += a1; p2 += a2; }
		}
	}
	if (seen) { p0 = fmaxf(fminf(p0, 1.0f), 0.f); p1 = fmaxf(fminf(p1, 1.0f), 0.f); p2 = fmaxf(fminf(p2, 1.0f), 0.f); }
	p[0] = p0; p[1] = p1; p[2] = p2;
	if (seen && !seen0) tmask[pe] = 1;
}

// ---- CylinderProject::project (stitch/warp.cc:25-44): thread per output pixel ----
// coltc[j] = (tan, cos) of the column's angle (j - offset.x) * sizefactor_inv, from the host libm (cyl_tables below)
struct CylParams { double cx, cy, offx, offy, sizefactor_inv; int r; };
template <typename T>       // T: float (Mat32f) or unsigned char (decoder bytes, interpolate_u8)
__global__ void __launch_bounds__(256) k_cyl_project(CylParams P, const double2* __restrict__ coltc, const T* __restrict__ img, int h, int w,
		float* __restrict__ out, int nh, int nw) {
	const int j = blockIdx.x * 64 + (threadIdx.x & 63);
	const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (i >= nh || j >= nw) return;
	const double py = ((double)i - P.offy) * P.sizefactor_inv;
	const double2 tc = coltc[j];
	const double ox = (double)P.r * tc.x + P.cx;                    // proj_r (warp.cc:19-23)
	const double oy = py * (double)P.r / tc.y + P.cy;
	float c[3] = {-1.f, -1.f, -1.f};
	// between(a, b, c) = a >= b && a <= c - 1 (lib/utils.hh:27)
	if (ox >= 0 && ox <= (double)(w - 1) && oy >= 0 && oy <= (double)(h - 1))
		source_interpolate(img, h, w, (float)oy, (float)ox, c);
	float* p = out + ((long long)i * nw + j) * 3;
	p[0] = c[0]; p[1] = c[1]; p[2] = c[2];
}

// ---- crop (lib/imgproc.cc:200-235): the largest rectangle of valid pixels ----
// Stage 1: column histograms.  height[line][k] = number of consecutive valid pixels ending at
// (line, k); thread per column walks the lines (coalesced across k).
__global__ void __launch_bounds__(256) k_crop_heights(const float* __restrict__ mat, int h, int w, int* __restrict__ height) {
	const int k = blockIdx.x * 256 + threadIdx.x;
	if (k >= w) return;
	int run = 0;
	for (int line = 0; line < h; ++line) {
		const float* p = mat + ((long long)line * w + k) * 3;
		const float m = fmaxf(fmaxf(p[0], p[1]), p[2]);
		run = m < 0 ? 0 : run + 1;                        // find Color::NO (:209)
		height[(long long)line * w + k] = run;
	}
}
// Stage 2: per line, the largest rectangle under the histogram.  left/right of the reference's
// pointer-jumping loops (:212-221) are the extents over which height >= height[k]; each thread
// finds them with a two-level search (own 64-chunk, chunk minima, target chunk).  The block's
// best (area, k) keeps the reference's first-maximum rule (:222-224: strict update in k order).
constexpr int CROP_CHUNK = 64;
__global__ void __launch_bounds__(256) k_crop_lines(const int* __restrict__ height, int h, int w, int4* __restrict__ line_best) {
	extern __shared__ int s_crop[];
	int* hs = s_crop;                    // w heights of this line
	int* cmin = hs + w;                  // minima of 64-chunks
	__shared__ int s_area[256], s_k[256], s_l[256], s_r[256];
	const int line = blockIdx.x, tid = threadIdx.x;
	const int nchunk = (w + CROP_CHUNK - 1) / CROP_CHUNK;
	for (int k = tid; k < w; k += 256) hs[k] = height[(long long)line * w + k];
	__syncthreads();
	for (int c = tid; c < nchunk; c += 256) {
		int m = 0x7fffffff;
		for (int k = c * CROP_CHUNK; k < w && k < (c + 1) * CROP_CHUNK; ++k) m = hs[k] < m ? hs[k] : m;
		cmin[c] = m;
	}
	__syncthreads();
	int barea = 0, bk = 0x7fffffff, bl = 0, br = 0;
	for (int k = tid; k < w; k += 256) {
		const int hk = hs[k];
		if (hk == 0) continue;                           // area 0 never beats maxarea (strict >, initial 0)
		// left: first j < k with hs[j] < hk, +1
		int j = k - 1;
		const int c0 = k / CROP_CHUNK;
		while (j >= c0 * CROP_CHUNK && hs[j] >= hk) --j;
		if (j < c0 * CROP_CHUNK && j >= 0) {
			int c = c0 - 1;
			while (c >= 0 && cmin[c] >= hk) --c;
			if (c < 0) j = -1;
			else { j = (c + 1) * CROP_CHUNK - 1; while (hs[j] >= hk) --j; }
		}
		const int left = j + 1;
		// right: first j > k with hs[j] < hk, -1
		j = k + 1;
		const int cend = (c0 + 1) * CROP_CHUNK < w ? (c0 + 1) * CROP_CHUNK : w;
		while (j < cend && hs[j] >= hk) ++j;
		if (j >= cend && j < w) {
			int c = c0 + 1;
			while (c < nchunk && cmin[c] >= hk) ++c;
			if (c >= nchunk) j = w;
			else { j = c * CROP_CHUNK; while (hs[j] >= hk) ++j; }
		}
		const int right = j - 1;
		const int area = (right - left + 1) * hk;
		if (area > barea) { barea = area; bk = k; bl = left; br = right; }   // ascending k per thread: first max
	}
	s_area[tid] = barea; s_k[tid] = bk; s_l[tid] = bl; s_r[tid] = br;
	__syncthreads();
	for (int st = 128; st > 0; st >>= 1) {
		if (tid < st) {
			const int oa = s_area[tid + st], ok = s_k[tid + st];
			if (oa > s_area[tid] || (oa == s_area[tid] && ok < s_k[tid])) { s_area[tid] = oa; s_k[tid] = ok; s_l[tid] = s_l[tid + st]; s_r[tid] = s_r[tid + st]; }
		}
		__syncthreads();
	}
	if (tid == 0) line_best[line] = make_int4(s_area[0], s_l[0], s_r[0], s_area[0] > 0 ? hs[s_k[0]] : 0);
}
// Stage 3: first line with the maximal area (update_max is strict, lines ascend)
__global__ void __launch_bounds__(256) k_crop_pick(const int4* __restrict__ line_best, int h, int* __restrict__ rect /* x0,y0,w,h */) {
	__shared__ int s_area[256], s_line[256];
	int ba = 0, bl = 0x7fffffff;
	for (int l = threadIdx.x; l < h; l += 256) { const int a = line_best[l].x; if (a > ba) { ba = a; bl = l; } }
	s_area[threadIdx.x] = ba; s_line[threadIdx.x] = bl;
	__syncthreads();
	for (int st = 128; st > 0; st >>= 1) {
		if (threadIdx.x < st) {
			const int oa = s_area[threadIdx.x + st], ol = s_line[threadIdx.x + st];
			if (oa > s_area[threadIdx.x] || (oa == s_area[threadIdx.x] && ol < s_line[threadIdx.x])) { s_area[threadIdx.x] = oa; s_line[threadIdx.x] = ol; }
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		if (s_area[0] <= 0) { rect[0] = 0; rect[1] = 1; rect[2] = 1; rect[3] = 0; }     // ll = rr = hh = nl = 0 (:205)
		else {
			const int4 b = line_best[s_line[0]];
			rect[0] = b.y; rect[1] = s_line[0] - b.w + 1; rect[2] = b.z - b.y + 1; rect[3] = b.w;
		}
	}
}
__global__ void __launch_bounds__(256) k_crop_copy(const float* __restrict__ src, int sw, int x0, int y0, float* __restrict__ dst, int dh, int dw) {
	const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
	if (e >= (long long)dh * dw * 3) return;
	const int row = (int)(e / (dw * 3)), c = (int)(e % (dw * 3));
	dst[e] = src[((long long)(row + y0) * sw + x0) * 3 + c];
}
// write_rgb / write_png quantisation (lib/imgio.cc:25-40,98-113): Color::NO -> white, float * 255 truncated
__global__ void __launch_bounds__(256) k_to_u8(const float* __restrict__ src, long long n, unsigned char* __restrict__ dst) {
	const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
	if (e >= n) return;
	const float v = src[e];
	dst[e] = (unsigned char)((v < 0 ? 1.f : v) * 255.f);
}

// ------------------------------- host geometry (fp64, host libm) -------------------------------
// Eigen::FullPivLU 3x3 inverse used by Homography::inverse (stitch/homography.cc:25-39)
bool inverse3_host(const double a[9], double inv[9]) {
	double lu[9]; memcpy(lu, a, sizeof(lu));
	int rowt[3], colt[3], nonzero = 3; double maxpivot = 0;
	for (int k = 0; k < 3; ++k) {
		int br = k, bc = k; double best = -1;
		for (int i = k; i < 3; ++i) for (int j = k; j < 3; ++j) { double v = std::fabs(lu[i * 3 + j]); if (v > best) { best = v; br = i; bc = j; } }
		if (best == 0.0) { nonzero = k; for (int i = k; i < 3; ++i) rowt[i] = colt[i] = i; break; }
		if (best > maxpivot) maxpivot = best;
		rowt[k] = br; colt[k] = bc;
		if (br != k) for (int j = 0; j < 3; ++j) std::swap(lu[k * 3 + j], lu[br * 3 + j]);
		if (bc != k) for (int i = 0; i < 3; ++i) std::swap(lu[i * 3 + k], lu[i * 3 + bc]);
		for (int i = k + 1; i < 3; ++i) lu[i * 3 + k] /= lu[k * 3 + k];
		for (int i = k + 1; i < 3; ++i) for (int j = k + 1; j < 3; ++j) lu[i * 3 + j] -= lu[i * 3 + k] * lu[k * 3 + j];
	}
	const double thr = std::fabs(maxpivot) * (DBL_EPSILON * 3);
	int rank = 0;
	for (int i = 0; i < nonzero; ++i) rank += (std::fabs(lu[i * 3 + i]) > thr);
	if (rank != 3) return false;
	for (int col = 0; col < 3; ++col) {
		double c[3];
		for (int i = 0; i < 3; ++i) c[i] = (i == col) ? 1.0 : 0.0;
		for (int i = 0; i < 3; ++i) std::swap(c[i], c[rowt[i]]);
		for (int i = 0; i < 3; ++i) for (int j = 0; j < i; ++j) c[i] -= lu[i * 3 + j] * c[j];
		for (int i = 2; i >= 0; --i) { for (int j = i + 1; j < 3; ++j) c[i] -= lu[i * 3 + j] * c[j]; c[i] /= lu[i * 3 + i]; }
		for (int i = 2; i >= 0; --i) std::swap(c[i], c[colt[i]]);
		for (int i = 0; i < 3; ++i) inv[i * 3 + col] = c[i];
	}
	return true;
}

void htrans_host(const double* d, double x, double y, double z, double out[3]) {
	out[0] = d[0] * x + d[1] * y + d[2] * z;
	out[1] = d[3] * x + d[4] * y + d[5] * z;
	out[2] = d[6] * x + d[7] * y + d[8] * z;
}
void homo2proj_host(int method, const double h[3], double out[2]) {   // projection.hh:16-18,33-36,48-51
	if (method == 0) { out[0] = h[0] / h[2]; out[1] = h[1] / h[2]; }
	else if (method == 1) { out[0] = std::atan2(h[0], h[2]); out[1] = h[1] / (std::hypot(h[0], h[2])); }
	else { out[0] = std::atan2(h[0], h[2]); out[1] = std::atan2(h[1], std::hypot(h[0], h[2])); }
}

void roi_of(const op_blend_geom* g, const double* range, int roi[4]) {   // Coor(double, double) truncation
	roi[0] = (int)((range[0] - g->proj_min[0]) / g->resolution[0]);
	roi[1] = (int)((range[1] - g->proj_min[1]) / g->resolution[1]);
	roi[2] = (int)((range[2] - g->proj_min[0]) / g->resolution[0]);
	roi[3] = (int)((range[3] - g->proj_min[1]) / g->resolution[1]);
}

// GaussCache (feature/gaussian.cc:17-40)
int gauss_taps(float sigma, int window_factor, BlurTaps& t) {
	int kw = (int)(std::ceil(0.3 * (sigma / 2 - 1) + 0.8) * window_factor);
	if (kw % 2 == 0) kw++;
	const int center = kw / 2;
	if (center > OP_MAX_KCENTER || kw < 1) return -1;
	float* kernel = &t.k[center];
	kernel[0] = 1;
	float exp_coeff = (float)(-1.0 / (sigma * sigma * 2)), wsum = 1;
	for (int i = 1; i <= center; i++)
		wsum += (kernel[i] = std::exp((float)(i * i) * exp_coeff)) * 2;
	float fac = (float)(1.0 / wsum);
	kernel[0] = fac;
	for (int i = 1; i <= center; i++) kernel[-i] = (kernel[i] *= fac);
	t.center = center;
	return 0;
}

struct CylProj { double cx, cy; int r, sizefactor; };
CylProj cyl_projector(int w, int h, double h_factor, float focal_length) {   // warp.cc:70-75
	CylProj p;
	p.r = (int)(std::hypot((double)w, (double)h) * (focal_length / 43.266));
	p.cx = w / 2; p.cy = h / 2 * h_factor;
	p.sizefactor = p.r;
	return p;
}
void cyl_proj(const CylProj& P, double px, double py, double out[2]) {       // warp.cc:13-17
	out[0] = std::atan((px - P.cx) / P.r);
	out[1] = (py - P.cy) / (std::hypot(px - P.cx, (double)P.r));
}

// The transcendentals of the canvas -> space map, evaluated by the host libm exactly where the reference evaluates
// them (stitcher_image.cc:144-145 + projection.hh:38-40,66-68): per column j  sin / cos of  j * resolution.x + min.x,
// per row i  tan of  i * resolution.y + min.y  (spherical) or that value itself (cylindrical).  (w1, h1) = canvas + 1.
// Layout: [w1 x (sin, cos)][h1 x row value].  Kept on the context while the geometry stays the same.
hipError_t trig_tables(op_ctx* ctx, const BlendGeom& g, int w1, int h1, BlendTrig* out) {
	op_ctx::TrigTables& T = ctx->blend_trig;
	const bool hit = T.method == g.method && T.w1 == w1 && T.h1 == h1 && T.minx == g.minx && T.miny == g.miny && T.resx == g.resx && T.resy == g.resy && T.dev.p;
	if (!hit) {
		T.method = -1;
		T.host.resize((size_t)2 * w1 + h1);
		double* col = T.host.data(); double* row = col + (size_t)2 * w1;
		const int chunks = (w1 + h1 + 1023) / 1024;
		auto fill = [&](int c) {
			const int a = c * 1024, b = std::min(w1 + h1, a + 1024);
			for (int e = a; e < b; ++e) {
				if (e < w1) { const double x = (double)e * g.resx + g.minx; col[2 * e] = std::sin(x); col[2 * e + 1] = std::cos(x); }
				else { const int i = e - w1; const double y = (double)i * g.resy + g.miny; row[i] = g.method == 2 ? std::tan(y) : y; }
			}
		};
		if (chunks > 2) host_parallel_for(chunks, fill); else for (int c = 0; c < chunks; ++c) fill(c);
		hipError_t e = T.dev.ensure(sizeof(double) * T.host.size());
		if (e != hipSuccess) return e;
		e = hipMemcpyAsync(T.dev.p, T.host.data(), sizeof(double) * T.host.size(), hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the host vector may be rewritten by the next miss
		if (e != hipSuccess) return e;
		T.method = g.method; T.w1 = w1; T.h1 = h1; T.minx = g.minx; T.miny = g.miny; T.resx = g.resx; T.resy = g.resy;
	}
	out->colsc = (const double2*)T.dev.p; out->rowt = (const double*)T.dev.p + (size_t)2 * w1; out->w1 = w1; out->h1 = h1;
	return hipSuccess;
}
// CylinderProject::project's per-column tan / cos (warp.cc:19-23,31): [nw x (tan, cos)]
hipError_t cyl_tables(op_ctx* ctx, double offx, double sizefactor_inv, int nw, const double2** out) {
	op_ctx::TrigTables& T = ctx->cyl_trig;
	const bool hit = T.method == 3 && T.w1 == nw && T.minx == offx && T.resx == sizefactor_inv && T.dev.p;
	if (!hit) {
		T.method = -1;
		T.host.resize((size_t)2 * nw);
		double* col = T.host.data();
		for (int j = 0; j < nw; ++j) { const double px = ((double)j - offx) * sizefactor_inv; col[2 * j] = std::tan(px); col[2 * j + 1] = std::cos(px); }
		hipError_t e = T.dev.ensure(sizeof(double) * T.host.size());
		if (e != hipSuccess) return e;
		e = hipMemcpyAsync(T.dev.p, T.host.data(), sizeof(double) * T.host.size(), hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) return e;
		T.method = 3; T.w1 = nw; T.minx = offx; T.resx = sizefactor_inv;
	}
	*out = (const double2*)T.dev.p;
	return hipSuccess;
}

}	// namespace

extern "C" {

int op_blend_prepare(const op_config* cfg, int proj_method, int identity_idx, int n, const int* shapes_wh,
		const double* homo, op_blend_geom* g, double* homo_inv, double* ranges) {
	if (!cfg || !shapes_wh || !homo || !g || !homo_inv || !ranges || n <= 0 || identity_idx < 0 || identity_idx >= n ||
			proj_method < 0 || proj_method > 2)
		OP_FAIL(OP_ERR_INVALID, "op_blend_prepare: bad argument");
	for (int i = 0; i < n; ++i)
		if (!inverse3_host(homo + 9 * i, homo_inv + 9 * i))
			OP_FAIL(OP_ERR_INVALID, "op_blend_prepare: homography " + std::to_string(i) + " is not invertible (homography.cc:33)");
	const int CORNER_SAMPLE = 100;        // stitcher_image.cc:43
	std::vector<double> cx, cy;
	for (int i = 0; i < CORNER_SAMPLE; ++i) {
		const double xi = (double)i / CORNER_SAMPLE - 0.5;
		cx.push_back(xi); cy.push_back(-0.5);
		cx.push_back(xi); cy.push_back(0.5);
	}
	for (int j = 0; j < CORNER_SAMPLE; ++j) {
		const double yj = (double)j / CORNER_SAMPLE - 0.5;
		cx.push_back(-0.5); cy.push_back(yj);
		cx.push_back(0.5); cy.push_back(yj);
	}
	double pmin[2] = {DBL_MAX, DBL_MAX}, pmax[2] = {-DBL_MAX, -DBL_MAX};
	for (int m = 0; m < n; ++m) {
		const int w = shapes_wh[2 * m], h = shapes_wh[2 * m + 1];
		double nmin[2] = {DBL_MAX, DBL_MAX}, nmax[2] = {-DBL_MAX, -DBL_MAX};
		for (size_t k = 0; k < cx.size(); ++k) {
			double hv[3], t[2];
			htrans_host(homo + 9 * m, cx[k] * w, cy[k] * h, 1, hv);
			homo2proj_host(proj_method, hv, t);
			for (int c = 0; c < 2; ++c) { if (t[c] < nmin[c]) nmin[c] = t[c]; if (nmax[c] < t[c]) nmax[c] = t[c]; }
		}
		ranges[4 * m] = nmin[0]; ranges[4 * m + 1] = nmin[1]; ranges[4 * m + 2] = nmax[0]; ranges[4 * m + 3] = nmax[1];
		for (int c = 0; c < 2; ++c) { if (nmin[c] < pmin[c]) pmin[c] = nmin[c]; if (pmax[c] < nmax[c]) pmax[c] = nmax[c]; }
	}
	g->proj_method = proj_method;
	g->proj_min[0] = pmin[0]; g->proj_min[1] = pmin[1]; g->proj_max[0] = pmax[0]; g->proj_max[1] = pmax[1];
	// get_final_resolution (stitcher_image.cc:79-114)
	const int refw = shapes_wh[2 * identity_idx], refh = shapes_wh[2 * identity_idx + 1];
	double c2[3], c1[3], p2[2], p1[2];
	htrans_host(homo + 9 * identity_idx, refw / 2.0, refh / 2.0, 1, c2);
	htrans_host(homo + 9 * identity_idx, -refw / 2.0, -refh / 2.0, 1, c1);
	homo2proj_host(proj_method, c2, p2); homo2proj_host(proj_method, c1, p1);
	double rx = p2[0] - p1[0], ry = p2[1] - p1[1];
	if (proj_method != 0) {
		if (rx < 0) rx = 2 * M_PI + rx;
		if (ry < 0) ry = M_PI + ry;
	}
	double resx = std::fabs(rx) / (double)refw, resy = std::fabs(ry) / (double)refh;
	const double tsx = (pmax[0] - pmin[0]) / resx, tsy = (pmax[1] - pmin[1]) / resy;
	const double max_edge = std::max(tsx, tsy);
	if (max_edge > 80000 || tsx * tsy > 1e9)
		OP_FAIL(OP_ERR_INVALID, "Target size too large. Looks like a stitching failure!");   // stitcher_image.cc:105-106
	if (max_edge > cfg->MAX_OUTPUT_SIZE) {
		const float ratio = (float)(max_edge / cfg->MAX_OUTPUT_SIZE);
		resx *= ratio; resy *= ratio;
	}
	g->resolution[0] = resx; g->resolution[1] = resy;
	return OP_OK;
}

int op_blend_canvas_dims(const op_blend_geom* g, const op_blend_image* imgs, int n, int* h, int* w) {
	if (!g || !imgs || n <= 0 || !h || !w) OP_FAIL(OP_ERR_INVALID, "op_blend_canvas_dims: bad argument");
	int tx = 0, ty = 0;       // Coor target_size{0,0}; update_max(bottom_right) (blender.cc:21)
	for (int i = 0; i < n; ++i) {
		int roi[4]; roi_of(g, imgs[i].range, roi);
		tx = std::max(tx, roi[2]); ty = std::max(ty, roi[3]);
	}
	*h = ty; *w = tx;
	return OP_OK;
}

}	// extern "C"

namespace {
// The op_blend_image array on the device as BlendImg (host images are uploaded; the uploads belong to own).  `who`
// prefixes the error messages.
int upload_images(op_ctx* ctx, const char* who, const op_blend_geom* g, const op_blend_image* imgs, int n, CallBlocks& own,
		std::vector<BlendImg>& h_imgs, long long& roi_total, long long& max_roi, bool& any_u8, BlendImg** d_out) {
	hipStream_t st = ctx->stream;
	const std::string w = who;
	h_imgs.assign(n, BlendImg{});
	roi_total = 0; max_roi = 0; any_u8 = false;      // any_u8: the set holds a byte view (the U8 kernel instances)
	for (int k = 0; k < n; ++k)       // the flag word, before any device work
		if (imgs[k].on_device & ~(OP_SRC_DEVICE | OP_SRC_U8)) OP_FAIL(OP_ERR_INVALID, w + ": unknown source flag on image " + std::to_string(k));
	for (int k = 0; k < n; ++k) {
		const op_blend_image& s = imgs[k];
		if (!s.data || s.h < 2 || s.w < 2) OP_FAIL(OP_ERR_INVALID, w + ": bad image " + std::to_string(k));
		BlendImg& b = h_imgs[k];
		b.h = s.h; b.w = s.w;
		b.mh = s.mat_h > 0 ? s.mat_h : s.h; b.mw = s.mat_w > 0 ? s.mat_w : s.w;
		if (b.mh < 2 || b.mw < 2) OP_FAIL(OP_ERR_INVALID, w + ": bad pixel buffer size of image " + std::to_string(k));
		b.u8 = (s.on_device & OP_SRC_U8) ? 1 : 0; any_u8 = any_u8 || b.u8;
		if (s.on_device & OP_SRC_DEVICE) b.data = s.data;
		else {            // a host view goes up in the type it has: 3 h w bytes, or 12 h w
			const size_t bytes = (b.u8 ? 1 : sizeof(float)) * 3 * (size_t)b.mh * b.mw;
			void* d = nullptr;
			HIPCHK(own.alloc(&d, bytes));
			HIPCHK(hipMemcpyAsync(d, s.data, bytes, hipMemcpyHostToDevice, st));
			b.data = d;
		}
		int roi[4]; roi_of(g, s.range, roi);
		if (roi[0] < 0 || roi[1] < 0 || roi[2] < roi[0] || roi[3] < roi[1]) OP_FAIL(OP_ERR_INVALID, w + ": image range outside proj_range");
		b.x0 = roi[0]; b.y0 = roi[1]; b.x1 = roi[2]; b.y1 = roi[3];
		memcpy(b.hinv, s.homo_inv, sizeof(b.hinv));
		b.rw = roi[2] - roi[0] + 1; b.rh = roi[3] - roi[1] + 1;      // Range::width/height, inclusive
		b.roi_off = roi_total; roi_total += (long long)b.rw * b.rh;
		max_roi = std::max(max_roi, (long long)b.rw * b.rh);
	}
	BlendImg* d_imgs = nullptr;
	HIPCHK(own.alloc(&d_imgs, sizeof(BlendImg) * n));
	HIPCHK(hipMemcpyAsync(d_imgs, h_imgs.data(), sizeof(BlendImg) * n, hipMemcpyHostToDevice, st));
	*d_out = d_imgs;
	return OP_OK;
}

int check_blend_args(const char* who, const op_blend_geom* g) {
	if (g->proj_method < 0 || g->proj_method > 2) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": bad projection method");
	if (!(g->resolution[0] > 0) || !(g->resolution[1] > 0)) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": resolution must be positive");
	return OP_OK;
}

// The blend of gain mode gm with the host table `gains`: GAIN_NONE (op_blend; no table), GAIN_IMAGE (op_blend_gains; n x 3),
// GAIN_BLOCK (op_blend_block_gains; n x gby x gbx x 3) or GAIN_VIGNETTE (op_blend_vignette; n x 3 gains then a1..a3)
int blend_impl(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int gm, const float* gains,
		int gbx, int gby, const char* who, op_canvas** out) {
	int rc = check_blend_args(who, g);
	if (rc != OP_OK) return rc;
	// multiband: the blur of every level but the last (GaussCache), checked before any allocation or launch -- a refusal
	// after them would hand blocks still being written back to the process-wide pool, which does not track streams
	std::vector<BlurTaps> level_taps(cfg->MULTIBAND > 1 ? cfg->MULTIBAND - 1 : 0);
	for (int level = 0; level < (int)level_taps.size(); ++level) {
		memset(&level_taps[level], 0, sizeof(BlurTaps));
		if (gauss_taps((float)(std::sqrt(level * 2 + 1.0) * 4), cfg->GAUSS_WINDOW_FACTOR, level_taps[level]) != 0)
			OP_FAIL(OP_ERR_UNSUPPORTED, std::string(who) + ": Gaussian kernel wider than 31 taps");
	}
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	int H, W;
	rc = op_blend_canvas_dims(g, imgs, n, &H, &W);
	if (rc != OP_OK) return rc;
	if (H <= 0 || W <= 0) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": empty canvas");
	CallBlocks own({ctx->stream});
	std::vector<BlendImg> h_imgs;
	long long roi_total = 0, max_roi = 0; bool any_u8 = false;
	BlendImg* d_imgs = nullptr;
	rc = upload_images(ctx, who, g, imgs, n, own, h_imgs, roi_total, max_roi, any_u8, &d_imgs);
	if (rc != OP_OK) return rc;
	float* d_gains = nullptr;
	if (gm != GAIN_NONE) {       // the whole table, once per call
		const size_t ng = gm == GAIN_VIGNETTE ? 3 * (size_t)n + 3 : 3 * (size_t)n * (gm == GAIN_BLOCK ? (size_t)gbx * gby : 1);
		HIPCHK(own.alloc(&d_gains, sizeof(float) * ng));
		HIPCHK(hipMemcpyAsync(d_gains, gains, sizeof(float) * ng, hipMemcpyHostToDevice, st));
	}
	float* canvas = nullptr;
	if (own.alloc(&canvas, sizeof(float) * 3 * (size_t)H * W) != hipSuccess) OP_FAIL(OP_ERR_HIP, std::string(who) + ": canvas allocation failed");
	const BlendGeom bg{g->proj_method, g->proj_min[0], g->proj_min[1], g->resolution[0], g->resolution[1]};
	const dim3 cgrid((W + 63) / 64, (H + 3) / 4);
	BlendTrig trig{nullptr, nullptr, 0, 0};
	if (bg.method != 0) {
		HostScope hs(ctx, "blend trig tables (host)");
		hipError_t e = trig_tables(ctx, bg, W + 1, H + 1, &trig);
		if (e != hipSuccess) OP_FAIL(OP_ERR_HIP, std::string(who) + ": trig tables: " + hipGetErrorString(e));
	}
	// the instances of the gain mode (gbx / gby are read by GAIN_BLOCK only)
	// and of the set's source types: the byte sampler is compiled into the U8 instances only, an all-fp32 call runs the others
	auto linear = k_blend_linear<GAIN_NONE, false>; auto first = k_mb_first_fused<GAIN_NONE, false>;
#define OP_GM_CASE(M) if (gm == M) { linear = any_u8 ? k_blend_linear<M, true> : k_blend_linear<M, false>; \
	first = any_u8 ? k_mb_first_fused<M, true> : k_mb_first_fused<M, false>; }
	OP_GM_CASE(GAIN_NONE) OP_GM_CASE(GAIN_IMAGE) OP_GM_CASE(GAIN_BLOCK) OP_GM_CASE(GAIN_VIGNETTE)
#undef OP_GM_CASE
	if (cfg->MULTIBAND <= 0) {
		ProfScope ps(ctx, "blend linear");
		hipLaunchKernelGGL(linear, cgrid, dim3(256), 0, st, bg, trig, d_imgs, n, canvas, H, W, cfg->ORDERED_INPUT, cfg->LAZY_READ, d_gains, gbx, gby);
		HIPCHK(hipGetLastError());
	} else {
		const int L = cfg->MULTIBAND;
		// every level's plane is kept when they fit comfortably (L x 16 bytes per ROI pixel: 0.2 GB per level for 38 views):
		// the bands are then applied in one pass over the canvas (k_mb_bands); otherwise two planes alternate and every
		// level has its own band pass
		const bool keep_all = L <= OP_MB_MAX_LEVELS && sizeof(float4) * (size_t)roi_total * (size_t)L <= ((size_t)64 << 30);
		const int nplanes = keep_all ? L : 2;
		std::vector<float4*> lv(nplanes, nullptr);
		float4* tmp = nullptr; unsigned char *mask = nullptr, *tmask = nullptr;
		for (int l = 0; l < nplanes; ++l) { HIPCHK(own.alloc(&lv[l], sizeof(float4) * roi_total)); }
		HIPCHK(own.alloc(&mask, roi_total));
		HIPCHK(own.alloc(&tmask, (size_t)H * W));
		const dim3 rgrid((unsigned)((max_roi + 255) / 256), n);
		{ ProfScope ps(ctx, "multiband first level");
		  const dim3 fgrid((W + 1 + 63) / 64, (H + 1 + 3) / 4);
		  hipLaunchKernelGGL(first, fgrid, dim3(256), 0, st, bg, trig, d_imgs, n, lv[0], mask, canvas, tmask, H, W, d_gains, gbx, gby);
		  HIPCHK(hipGetLastError()); }
		bool band0_done = false;                 // level 0's band written by the fused blur
		for (int level = 0; level < L; ++level) {
			const int is_last = (level == L - 1);
			float4* cur = keep_all ? lv[level] : lv[level & 1];
			float4* nxt = is_last ? nullptr : (keep_all ? lv[level + 1] : lv[(level + 1) & 1]);
			bool band_done = false;
			if (!is_last) {
				ProfScope ps(ctx, "multiband blur");
				const BlurTaps& taps = level_taps[level];
				if (taps.center == 6 || taps.center == 9) {       // shipped GAUSS_WINDOW_FACTOR: both passes in one kernel
					const int C = taps.center, two = 256 - 2 * C, segr = (C <= 6 ? 8 : 6) * (2 * C + 2);      // k_mb_blur_fused: SEG
					unsigned items = 1;
					for (int k = 0; k < n; ++k)
						items = std::max(items, (unsigned)(((h_imgs[k].rw + two - 1) / two) * ((h_imgs[k].rh + segr - 1) / segr)));
					band_done = level == 0;
					if (C == 6 && level == 0) hipLaunchKernelGGL((k_mb_blur_fused<6, true>), dim3(items, n), dim3(256), 0, st, d_imgs, taps, cur, nxt, canvas, tmask, H, W);
					else if (C == 6) hipLaunchKernelGGL((k_mb_blur_fused<6, false>), dim3(items, n), dim3(256), 0, st, d_imgs, taps, cur, nxt, canvas, tmask, H, W);
					else if (level == 0) hipLaunchKernelGGL((k_mb_blur_fused<9, true>), dim3(items, n), dim3(256), 0, st, d_imgs, taps, cur, nxt, canvas, tmask, H, W);
					else hipLaunchKernelGGL((k_mb_blur_fused<9, false>), dim3(items, n), dim3(256), 0, st, d_imgs, taps, cur, nxt, canvas, tmask, H, W);
				} else {
					if (!tmp) { HIPCHK(own.alloc(&tmp, sizeof(float4) * roi_total)); }
					hipLaunchKernelGGL((k_mb_blur<true, 0>), rgrid, dim3(256), 0, st, d_imgs, taps, cur, tmp);
					hipLaunchKernelGGL((k_mb_blur<false, 0>), rgrid, dim3(256), 0, st, d_imgs, taps, tmp, nxt);
				}
				HIPCHK(hipGetLastError());
			}
			if (level == 0) band0_done = band_done;
			if (!keep_all && !band_done) { ProfScope ps(ctx, "multiband band");
			  hipLaunchKernelGGL(k_mb_accumulate, cgrid, dim3(256), 0, st, d_imgs, n, cur, nxt, mask, canvas, tmask, H, W, is_last);
			  HIPCHK(hipGetLastError()); }
		}
		if (keep_all) {
			ProfScope ps(ctx, "multiband band");
			const int first = band0_done ? 1 : 0, NL = L - first;
			BandPlanes P; memset(&P, 0, sizeof(P));
			for (int l = 0; l < NL; ++l) P.lv[l] = lv[first + l];
			switch (NL) {
#define OP_MB_CASE(N) case N: hipLaunchKernelGGL((k_mb_bands<N>), cgrid, dim3(256), 0, st, d_imgs, n, P, mask, canvas, tmask, H, W); break;
				OP_MB_CASE(1) OP_MB_CASE(2) OP_MB_CASE(3) OP_MB_CASE(4) OP_MB_CASE(5) OP_MB_CASE(6)
#undef OP_MB_CASE
				default: break;
			}
			HIPCHK(hipGetLastError());
		}
	}
	HIPCHK(own.finish());
	resolve_profile(ctx);
	*out = new op_canvas{own.release(canvas), H, W, ctx->device};      // born owning its block, on the last line
	return OP_OK;
}

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

// The host side of op_gain_overlap, op_gain_block_overlap and op_vignette_overlap after their own checks: `entries` counts
// and entries x per values, zeroed on the device, filled by kernel(bg, trig, images, n, H, W, stride, LAZY_READ, extra...,
// counts, values) over the canvas lattice of `stride`, copied to count / values.  cap_lattice: more than VIG_MAX_LATTICE
// lattice points are refused (the bound of the vignetting sums).  kernel_u8: the instance for a set that holds a byte view.
template <typename K, typename... X>
int overlap_stats(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int stride, const char* who,
		const char* label, long long entries, int per, bool cap_lattice, int64_t* count, int64_t* values, K kernel, K kernel_u8, X... extra) {
	if (entries == 0) return OP_OK;                     // one image: no pair
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	int H, W;
	int rc = op_blend_canvas_dims(g, imgs, n, &H, &W);
	if (rc != OP_OK) return rc;
	if (H <= 0 || W <= 0) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": empty canvas");
	// a stride beyond the canvas leaves the lattice {(0, 0)} -- clamped so that lattice coordinates stay far from overflow
	stride = std::min(stride, std::max(H, W));
	const int hs_ = (H + stride - 1) / stride, ws_ = (W + stride - 1) / stride;
	if (cap_lattice && (long long)hs_ * ws_ > VIG_MAX_LATTICE)
		OP_FAIL(OP_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string((long long)hs_ * ws_) + " lattice points exceed 2^30 (raise the stride)");
	CallBlocks own({ctx->stream});
	std::vector<BlendImg> h_imgs;
	long long roi_total = 0, max_roi = 0; bool any_u8 = false;
	BlendImg* d_imgs = nullptr;
	rc = upload_images(ctx, who, g, imgs, n, own, h_imgs, roi_total, max_roi, any_u8, &d_imgs);
	if (rc != OP_OK) return rc;
	unsigned long long* d_stats = nullptr;         // entries counts, then entries x per values
	const size_t stat_bytes = sizeof(unsigned long long) * (1 + per) * (size_t)entries;
	HIPCHK(own.alloc(&d_stats, stat_bytes));
	HIPCHK(hipMemsetAsync(d_stats, 0, stat_bytes, st));
	const BlendGeom bg{g->proj_method, g->proj_min[0], g->proj_min[1], g->resolution[0], g->resolution[1]};
	BlendTrig trig{nullptr, nullptr, 0, 0};
	if (bg.method != 0) {            // the blend's own tables (same key: canvas + 1), so a following blend finds them cached
		HostScope hs(ctx, "blend trig tables (host)");
		HIPCHK(trig_tables(ctx, bg, W + 1, H + 1, &trig));
	}
	{ ProfScope ps(ctx, label);
	  hipLaunchKernelGGL(any_u8 ? kernel_u8 : kernel, dim3((ws_ + 63) / 64, (hs_ + 3) / 4), dim3(256), sizeof(unsigned long long) * ((n + 63) / 64), st,
	                     bg, trig, d_imgs, n, H, W, stride, cfg->LAZY_READ, extra..., d_stats, d_stats + entries);
	  HIPCHK(hipGetLastError()); }
	HIPCHK(hipMemcpyAsync(count, d_stats, sizeof(int64_t) * (size_t)entries, hipMemcpyDeviceToHost, st));
	HIPCHK(hipMemcpyAsync(values, d_stats + entries, sizeof(int64_t) * per * (size_t)entries, hipMemcpyDeviceToHost, st));
	HIPCHK(own.finish());
	resolve_profile(ctx);
	return OP_OK;
}

}	// namespace

extern "C" {

int op_blend(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, op_canvas** out) {
	if (!ctx || !cfg || !g || !imgs || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_blend: bad argument");
	return blend_impl(ctx, cfg, g, imgs, n, GAIN_NONE, nullptr, 0, 0, "op_blend", out);
}

int op_blend_gains(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, const float* gains, op_canvas** out) {
	if (!ctx || !cfg || !g || !imgs || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_blend_gains: bad argument");
	const int rc = check_gains("op_blend_gains", gains, 3ll * n, 3);
	if (rc != OP_OK) return rc;
	return blend_impl(ctx, cfg, g, imgs, n, gains ? GAIN_IMAGE : GAIN_NONE, gains, 0, 0, "op_blend_gains", out);
}

int op_blend_block_gains(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int bx, int by,
		const float* gains, op_canvas** out) {
	if (!ctx || !cfg || !g || !imgs || n <= 0 || !out || bx < 1 || bx > GAIN_MAX_BLOCKS || by < 1 || by > GAIN_MAX_BLOCKS)
		OP_FAIL(OP_ERR_INVALID, "op_blend_block_gains: bad argument");
	const int rc = check_gains("op_blend_block_gains", gains, 3ll * n * bx * by, 3ll * bx * by);
	if (rc != OP_OK) return rc;
	return blend_impl(ctx, cfg, g, imgs, n, gains ? GAIN_BLOCK : GAIN_NONE, gains, bx, by, "op_blend_block_gains", out);
}

int op_blend_vignette(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, const float* gains,
		const float* poly, op_canvas** out) {
	if (!ctx || !cfg || !g || !imgs || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_blend_vignette: bad argument");
	int rc = check_lens_frame("op_blend_vignette", imgs, n);
	if (rc != OP_OK) return rc;
	rc = check_gains("op_blend_vignette", gains, 3ll * n, 3);
	if (rc != OP_OK) return rc;
	std::vector<float> table(3 * (size_t)n + 3, 1.f);   // gains (NULL = 1), then a1..a3 (NULL = 0)
	if (gains) std::copy(gains, gains + 3 * (size_t)n, table.begin());
	for (int j = 0; j < 3; ++j) table[3 * (size_t)n + j] = poly ? poly[j] : 0.f;
	const double a[3] = {table[3 * (size_t)n], table[3 * (size_t)n + 1], table[3 * (size_t)n + 2]};
	if (!vignette_curve_positive(a)) OP_FAIL(OP_ERR_INVALID, "op_blend_vignette: the curve is not finite and positive on [0, 1]");
	return blend_impl(ctx, cfg, g, imgs, n, GAIN_VIGNETTE, table.data(), 0, 0, "op_blend_vignette", out);
}

int op_vignette_overlap(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int stride,
		float clip, int64_t* count, int64_t* moments) {
	if (!ctx || !cfg || !g || !imgs || n < 1 || stride < 1 || !(clip > 0.f) || !(clip <= 1.f) || (n > 1 && (!count || !moments)))
		OP_FAIL(OP_ERR_INVALID, "op_vignette_overlap: bad argument");
	int rc = check_blend_args("op_vignette_overlap", g);
	if (rc != OP_OK) return rc;
	rc = check_lens_frame("op_vignette_overlap", imgs, n);
	if (rc != OP_OK) return rc;
	if (n > GAIN_MAX_IMAGES) OP_FAIL(OP_ERR_UNSUPPORTED, "op_vignette_overlap: more than " + std::to_string(GAIN_MAX_IMAGES) + " images");
	return overlap_stats(ctx, cfg, g, imgs, n, stride, "op_vignette_overlap", "vignette overlap", (long long)n * (n - 1) / 2, VIG_MOMENTS, true,
	                     count, moments, k_vignette_overlap<false>, k_vignette_overlap<true>, clip);
}

int op_gain_overlap(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int stride,
		int64_t* count, int64_t* sums) {
	if (!ctx || !cfg || !g || !imgs || n < 1 || stride < 1 || (n > 1 && (!count || !sums)))
		OP_FAIL(OP_ERR_INVALID, "op_gain_overlap: bad argument");
	const int rc = check_blend_args("op_gain_overlap", g);
	if (rc != OP_OK) return rc;
	if (n > GAIN_MAX_IMAGES) OP_FAIL(OP_ERR_UNSUPPORTED, "op_gain_overlap: more than " + std::to_string(GAIN_MAX_IMAGES) + " images");
	return overlap_stats(ctx, cfg, g, imgs, n, stride, "op_gain_overlap", "gain overlap", (long long)n * (n - 1) / 2, 6, false,
	                     count, sums, k_gain_overlap<false>, k_gain_overlap<true>);
}

}	// extern "C"

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

int op_gain_block_overlap(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int stride,
		int bx, int by, int64_t* count, int64_t* sums) {
	if (!ctx || !cfg || !g || !imgs || n < 1 || stride < 1 || bx < 1 || bx > GAIN_MAX_BLOCKS || by < 1 || by > GAIN_MAX_BLOCKS ||
			(n > 1 && (!count || !sums)))
		OP_FAIL(OP_ERR_INVALID, "op_gain_block_overlap: bad argument");
	const int rc = check_blend_args("op_gain_block_overlap", g);
	if (rc != OP_OK) return rc;
	if (n > GAIN_MAX_IMAGES) OP_FAIL(OP_ERR_UNSUPPORTED, "op_gain_block_overlap: more than " + std::to_string(GAIN_MAX_IMAGES) + " images");
	const long long npairs = (long long)n * (n - 1) / 2, nblk = (long long)bx * by, entries = npairs * nblk * nblk;
	if (entries > GAIN_BLOCK_MAX_ENTRIES)
		OP_FAIL(OP_ERR_UNSUPPORTED, "op_gain_block_overlap: " + std::to_string(entries) + " unit-pair entries (pairs x (bx by)^2) exceed " +
		        std::to_string(GAIN_BLOCK_MAX_ENTRIES));
	return overlap_stats(ctx, cfg, g, imgs, n, stride, "op_gain_block_overlap", "gain block overlap", entries, 6, false, count, sums,
	                     k_gain_block_overlap<false>, k_gain_block_overlap<true>, bx, by);
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

int op_canvas_dims(const op_canvas* c, int* h, int* w) {
	if (!c || !h || !w) OP_FAIL(OP_ERR_INVALID, "op_canvas_dims: bad argument");
	*h = c->h; *w = c->w; return OP_OK;
}
const float* op_canvas_device(const op_canvas* c) { return c ? c->data : nullptr; }
int op_canvas_copy(op_ctx* ctx, const op_canvas* c, float* host) {
	if (!ctx || !c || !host) OP_FAIL(OP_ERR_INVALID, "op_canvas_copy: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	HIPCHK(hipMemcpyAsync(host, c->data, sizeof(float) * 3 * (size_t)c->h * c->w, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return OP_OK;
}
void op_canvas_free(op_canvas* c) {
	if (!c) return;
	hipSetDevice(c->device);
	pool_free(c->data);
	delete c;
}

int op_canvas_crop(op_ctx* ctx, const op_canvas* c, op_canvas** out, int* x0, int* y0) {
	if (!ctx || !c || !out) OP_FAIL(OP_ERR_INVALID, "op_canvas_crop: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	const int h = c->h, w = c->w;
	if ((size_t)(w + (w + CROP_CHUNK - 1) / CROP_CHUNK) * sizeof(int) > 150 * 1024) OP_FAIL(OP_ERR_UNSUPPORTED, "op_canvas_crop: canvas wider than 38000 px");
	CallBlocks own({ctx->stream});
	int* d_height = nullptr; int4* d_best = nullptr; int* d_rect = nullptr;
	HIPCHK(own.alloc(&d_height, sizeof(int) * (size_t)h * w));
	HIPCHK(own.alloc(&d_best, sizeof(int4) * h));
	HIPCHK(own.alloc(&d_rect, sizeof(int) * 4));
	HIPCHK(hipFuncSetAttribute((const void*)k_crop_lines, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));   // idempotent
	int rect[4];
	{ ProfScope ps(ctx, "crop");
	  hipLaunchKernelGGL(k_crop_heights, dim3((w + 255) / 256), dim3(256), 0, st, c->data, h, w, d_height);
	  HIPCHK(hipGetLastError());
	  const size_t lds = sizeof(int) * (size_t)(w + (w + CROP_CHUNK - 1) / CROP_CHUNK);
	  hipLaunchKernelGGL(k_crop_lines, dim3(h), dim3(256), lds, st, d_height, h, w, d_best);
	  HIPCHK(hipGetLastError());
	  hipLaunchKernelGGL(k_crop_pick, dim3(1), dim3(256), 0, st, d_best, h, d_rect);
	  HIPCHK(hipGetLastError()); }
	HIPCHK(hipMemcpyAsync(rect, d_rect, sizeof(rect), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	const size_t n = (size_t)rect[3] * rect[2] * 3;
	float* data = nullptr;
	if (own.alloc(&data, sizeof(float) * (n ? n : 1)) != hipSuccess) OP_FAIL(OP_ERR_HIP, "op_canvas_crop: allocation failed");
	if (n) {
		hipLaunchKernelGGL(k_crop_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c->data, w, rect[0], rect[1], data, rect[3], rect[2]);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(st));
	}
	own.settled();
	resolve_profile(ctx);
	if (x0) *x0 = rect[0];
	if (y0) *y0 = rect[1];
	*out = new op_canvas{own.release(data), rect[3], rect[2], ctx->device};      // born owning its block, on the last line
	return OP_OK;
}

int op_canvas_copy_u8(op_ctx* ctx, const op_canvas* c, unsigned char* host) {
	if (!ctx || !c || !host) OP_FAIL(OP_ERR_INVALID, "op_canvas_copy_u8: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	const long long n = (long long)c->h * c->w * 3;
	if (n == 0) return OP_OK;
	CallBlocks own({ctx->stream});
	unsigned char* d = nullptr;
	HIPCHK(own.alloc(&d, (size_t)n));
	hipLaunchKernelGGL(k_to_u8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, c->data, n, d);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(host, d, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(own.finish());
	return OP_OK;
}

int op_cyl_warp_shape(const op_config* cfg, int w, int h, double h_factor, double* pts, int npts,
		int* new_w, int* new_h, double* offset) {
	if (!cfg || w < 2 || h < 2 || npts < 0 || (npts && !pts) || !new_w || !new_h || !offset)
		OP_FAIL(OP_ERR_INVALID, "op_cyl_warp_shape: bad argument");
	const CylProj P = cyl_projector(w, h, h_factor, cfg->FOCAL_LENGTH);
	if (P.r <= 0) OP_FAIL(OP_ERR_INVALID, "op_cyl_warp_shape: degenerate projector radius");
	// warp.cc:47-52 scans all w*h pixels.  x = atan((j-cx)/r) does not depend on i, and for a fixed
	// j the quotient y = (i-cy)/hypot(j-cx, r) is monotone in i in floating point as well (one
	// subtraction and one division by a fixed positive number), so rows 0 and h-1 hold both
	// extremes of every column: 2w evaluations give the identical min/max.
	double mn[2] = {DBL_MAX, DBL_MAX}, mx[2] = {0, 0};
	for (int j = 0; j < w; ++j) for (int e = 0; e < 2; ++e) {
		double c[2]; cyl_proj(P, j, e ? h - 1 : 0, c);
		for (int q = 0; q < 2; ++q) { if (c[q] < mn[q]) mn[q] = c[q]; if (mx[q] < c[q]) mx[q] = c[q]; }
	}
	for (int q = 0; q < 2; ++q) { mx[q] = mx[q] * P.sizefactor; mn[q] = mn[q] * P.sizefactor; }
	const double rsx = mx[0] - mn[0], rsy = mx[1] - mn[1];
	offset[0] = mn[0] * (-1); offset[1] = mn[1] * (-1);
	const int sx = (int)rsx, sy = (int)rsy;
	for (int k = 0; k < npts; ++k) {              // warp.cc:59-65
		double c[2];
		cyl_proj(P, pts[2 * k] + w / 2, pts[2 * k + 1] + h / 2, c);
		pts[2 * k] = c[0] * P.sizefactor + offset[0];
		pts[2 * k + 1] = c[1] * P.sizefactor + offset[1];
		pts[2 * k] -= sx / 2;
		pts[2 * k + 1] -= sy / 2;
	}
	*new_w = sx; *new_h = sy;
	return OP_OK;
}

int op_cyl_warp(op_ctx* ctx, const op_config* cfg, const op_image* img, double h_factor, op_canvas** out) {
	if (!ctx || !cfg || !img || !img->data || !out) OP_FAIL(OP_ERR_INVALID, "op_cyl_warp: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	int nw, nh; double off[2];
	int rc = op_cyl_warp_shape(cfg, img->w, img->h, h_factor, nullptr, 0, &nw, &nh, off);
	if (rc != OP_OK) return rc;
	if (nw <= 0 || nh <= 0) OP_FAIL(OP_ERR_INVALID, "op_cyl_warp: empty output");
	CallBlocks own({ctx->stream});
	if (img->dtype != OP_F32 && img->dtype != OP_U8) OP_FAIL(OP_ERR_INVALID, "op_cyl_warp: unknown dtype");
	const bool u8 = img->dtype == OP_U8;
	const void* src = img->data;
	if (!img->on_device) {
		const size_t bytes = (u8 ? 1 : sizeof(float)) * 3 * (size_t)img->h * img->w;
		void* d = nullptr;
		HIPCHK(own.alloc(&d, bytes));
		HIPCHK(hipMemcpyAsync(d, img->data, bytes, hipMemcpyHostToDevice, st));
		src = d;
	}
	const CylProj P = cyl_projector(img->w, img->h, h_factor, cfg->FOCAL_LENGTH);
	float* data = nullptr;
	if (own.alloc(&data, sizeof(float) * 3 * (size_t)nh * nw) != hipSuccess) OP_FAIL(OP_ERR_HIP, "op_cyl_warp: allocation failed");
	const CylParams cp{P.cx, P.cy, off[0], off[1], 1.0 / P.sizefactor, P.r};
	const double2* coltc = nullptr;
	{ hipError_t e = cyl_tables(ctx, cp.offx, cp.sizefactor_inv, nw, &coltc);
	  if (e != hipSuccess) OP_FAIL(OP_ERR_HIP, std::string("op_cyl_warp: trig table: ") + hipGetErrorString(e)); }
	{ ProfScope ps(ctx, "cylinder warp");
	  if (u8) hipLaunchKernelGGL(k_cyl_project<unsigned char>, dim3((nw + 63) / 64, (nh + 3) / 4), dim3(256), 0, st, cp, coltc, (const unsigned char*)src, img->h, img->w, data, nh, nw);
	  else hipLaunchKernelGGL(k_cyl_project<float>, dim3((nw + 63) / 64, (nh + 3) / 4), dim3(256), 0, st, cp, coltc, (const float*)src, img->h, img->w, data, nh, nw); }
	HIPCHK(hipGetLastError());
	HIPCHK(own.finish());
	resolve_profile(ctx);
	*out = new op_canvas{own.release(data), nh, nw, ctx->device};      // born owning its block, on the last line
	return OP_OK;
}

// ---- op_views: the views of a job, uploaded once in the type the decoder produced, resident for SIFT, the cylinder
// warp, the overlap passes and every blend (the reference's seam: ImageRef::load / img, stitch/imageref.hh:15-31) ----
int op_views_upload(op_ctx* ctx, const op_image* imgs, int n, op_views** out) {
	if (!ctx || !imgs || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_views_upload: bad argument");
	*out = nullptr;
	for (int i = 0; i < n; ++i)
		if (!imgs[i].data || imgs[i].h < 2 || imgs[i].w < 2 || (imgs[i].dtype != OP_F32 && imgs[i].dtype != OP_U8) ||
				(imgs[i].on_device != 0 && imgs[i].on_device != 1))
			OP_FAIL(OP_ERR_INVALID, "op_views_upload: bad image " + std::to_string(i));
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	// every view at an offset that is a multiple of 256 bytes of ONE block
	std::vector<size_t> bytes(n), off(n);
	size_t total = 0;
	for (int i = 0; i < n; ++i) {
		bytes[i] = (imgs[i].dtype == OP_U8 ? 1 : sizeof(float)) * 3 * (size_t)imgs[i].h * imgs[i].w;
		off[i] = total; total += (bytes[i] + 255) & ~(size_t)255;
	}
	CallBlocks own({st});
	char* block = nullptr;
	HIPCHK(own.alloc(&block, total));
	// host images of one size at one constant stride (a contiguous array of frames, a decoder pool) go up in ONE copy
	bool packed = n > 1;
	for (int i = 0; i < n && packed; ++i) packed = !imgs[i].on_device && bytes[i] == bytes[0];
	ptrdiff_t hstride = packed ? (const char*)imgs[1].data - (const char*)imgs[0].data : 0;
	packed = packed && hstride >= (ptrdiff_t)bytes[0];
	for (int i = 2; i < n && packed; ++i) packed = (const char*)imgs[i].data - (const char*)imgs[i - 1].data == hstride;
	hipError_t e = hipSuccess;
	if (packed) e = hipMemcpy2DAsync(block, off[1], imgs[0].data, (size_t)hstride, bytes[0], (size_t)n, hipMemcpyHostToDevice, st);
	else for (int i = 0; i < n && e == hipSuccess; ++i)
		e = hipMemcpyAsync(block + off[i], imgs[i].data, bytes[i], imgs[i].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = own.finish();       // the caller's host buffers are free again when this returns
	if (e != hipSuccess) OP_FAIL(OP_ERR_HIP, std::string("op_views_upload: ") + hipGetErrorString(e));
	op_views* v = new op_views;
	v->ctx = ctx; v->block = own.release(block);
	v->imgs.resize(n);
	for (int i = 0; i < n; ++i) v->imgs[i] = op_image{block + off[i], imgs[i].h, imgs[i].w, 1, imgs[i].dtype};
	*out = v;
	return OP_OK;
}

int op_views_count(const op_views* v) {
	if (!v) OP_FAIL(OP_ERR_INVALID, "op_views_count: NULL views");
	return (int)v->imgs.size();
}

int op_views_image(const op_views* v, int i, op_image* out) {
	if (!v || !out || i < 0 || i >= (int)v->imgs.size()) OP_FAIL(OP_ERR_INVALID, "op_views_image: bad argument");
	*out = v->imgs[i];
	return OP_OK;
}

int op_views_blend_image(const op_views* v, int i, op_blend_image* out) {
	if (!v || !out || i < 0 || i >= (int)v->imgs.size()) OP_FAIL(OP_ERR_INVALID, "op_views_blend_image: bad argument");
	const op_image& im = v->imgs[i];
	out->data = (const float*)im.data; out->h = im.h; out->w = im.w;
	out->on_device = OP_SRC_DEVICE | (im.dtype == OP_U8 ? OP_SRC_U8 : 0);
	out->mat_h = 0; out->mat_w = 0;
	return OP_OK;
}

void op_views_free(op_views* v) {
	if (!v) return;
	// the pool does not track streams: work of the context's stream that still reads the views must be over before the
	// block can be handed to another caller
	if (v->block) {
		if (hipSetDevice(v->ctx->device) == hipSuccess) (void)hipStreamSynchronize(v->ctx->stream);
		pool_free(v->block);
	}
	delete v;
}

}	// extern "C"
