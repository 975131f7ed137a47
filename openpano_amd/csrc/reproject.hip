// reproject.hip -- a finished equirectangular panorama looked at again, on the device (op_canvas_reproject): the reference's
// planet (main.cc:294-331), a rectilinear view in a chosen direction, and with six of those the faces of a cube.  Each is a
// gather from the canvas, one thread per output pixel.  tests/reproject_cases.py restates every map in numpy, one operation per
// call; the kernel equals it bit for bit because nothing here depends on a libm: the angle is pano_atan2 (pano_angle.hpp), the
// square roots are correctly rounded, the unit is built without contraction.  The host parts (the frame of a spherical canvas,
// the view specs, the refusals) are plain C++ in blend_geom.cc.
#include "blend_sample.hpp"
#include "pano_angle.hpp"

namespace {

// interpolate() (blend_sample.hpp) for a source whose columns close a full turn: the same fp32 sequence, with the column bound
// c <= cols instead of c < cols - 1; a right tap at column cols reads column 0, and a c that narrowed to exactly cols reads
// column 0 with fraction 0.  Rows are unchanged.
// Reads stay inside [img, img + 3 rows cols): the test admits 0 <= r < rows - 1 and 0 <= c <= cols only (a NaN fails it), and
// both bounds are exact as floats because op_canvas_reproject refuses sources beyond 2^24 rows or columns; so fr = floor(r)
// lies in [0, rows - 2] and fr + 1 in [1, rows - 1]; fc = floor(c) lies in [0, cols], cols itself is replaced by 0, which
// leaves fc in [0, cols - 1]; and fc1 is fc + 1 <= cols - 1, or 0.
__device__ __forceinline__ bool interpolate_wrap(const float* __restrict__ img, int rows, int cols, float r, float c, float (&out)[3]) {
	if (!(r >= 0.f && c >= 0.f && r < (float)(rows - 1) && c <= (float)cols)) return false;
	const int fr = (int)floorf(r);
	int fc = (int)floorf(c);
	r -= (float)fr; c -= (float)fc;
	if (fc >= cols) { fc = 0; c = 0.f; }
	const int fc1 = fc + 1 == cols ? 0 : fc + 1;
	const float* row0 = img + (long long)fr * cols * 3;
	const float* row1 = row0 + (long long)cols * 3;
	const float* p00 = row0 + fc * 3; const float* p01 = row0 + fc1 * 3;
	const float* p10 = row1 + fc * 3; const float* p11 = row1 + fc1 * 3;
	float a0 = p00[0], a1 = p00[1], a2 = p00[2];
	if (a0 < 0) return false;
	float b0 = p10[0], b1 = p10[1], b2 = p10[2];
	if (b0 < 0) return false;
	float c0 = p11[0], c1 = p11[1], c2 = p11[2];
	if (c0 < 0) return false;
	float d0 = p01[0], d1 = p01[1], d2 = p01[2];
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

// Thread per output pixel, 64 x 4 tiles as k_canvas_perspective.  F and S travel by value in the kernel arguments.
template <int MODE, bool WRAP>
__global__ void __launch_bounds__(256) k_canvas_reproject(op_pano_frame F, op_view_spec S, const float* __restrict__ src, int H, int W,
		float* __restrict__ out) {
	const int j = blockIdx.x * 64 + (threadIdx.x & 63);
	const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (i >= S.out_h || j >= S.out_w) return;
	float col[3];
	bool ok = false;
	if (H < 1 || W < 1) {
		// an empty source: nothing to sample
	} else if (MODE == OP_VIEW_PLANET) {                   // main.cc:297-329, operation by operation
		const int center = S.out_w / 2;
		const int di = center - i, dj = center - j;
		double dist = sqrt((double)((long long)di * di + (long long)dj * dj));      // hypot(center - i, center - j)
		if (!(dist >= (double)center || dist == 0)) {
			dist = dist / (double)center;
			dist = (double)H - dist * (double)H;
			double theta;
			if (j == center) theta = i < center ? PANO_PI / 2 : 3 * PANO_PI / 2;
			else {
				theta = pano_atan2((double)di / (double)dj, 1.0);       // atan(q)
				if (theta < 0) theta += PANO_PI;
				if (theta == 0 && j > center) theta += PANO_PI;
				if (center < i) theta += PANO_PI;
			}
			theta = theta / (PANO_PI * 2) * (double)W;
			if ((double)(H - 1) < dist) dist = (double)(H - 1);     // update_min(dist, h - 1)
			// interpolate(const Mat32f&, float, float): both narrow at the call
			ok = WRAP ? interpolate_wrap(src, H, W, (float)dist, (float)theta, col) : interpolate(src, H, W, (float)dist, (float)theta, col);
		}
	} else {
		const double u = (double)j - 0.5 * (double)(S.out_w - 1), v = (double)i - 0.5 * (double)(S.out_h - 1);
		const double* R = S.rot;
		const double dx = R[0] * u + R[1] * v + R[2] * S.focal;
		const double dy = R[3] * u + R[4] * v + R[5] * S.focal;
		const double dz = R[6] * u + R[7] * v + R[8] * S.focal;
		const double lon = pano_atan2(dx, dz);
		const double lat = pano_atan2(dy, sqrt(dx * dx + dz * dz));
		const double py = (lat - F.lat0) / F.step_lat;
		if (WRAP) {
			double d = lon - F.lon0;                             // in [-2 pi, 2 pi]: one correction brings it into [0, 2 pi)
			if (d < 0) d = d + PANO_2PI;
			if (d >= PANO_2PI) d = d - PANO_2PI;
			const double px = d / (PANO_PI * 2) * (double)W;
			if (!(py < 0 || py >= H) && !(px != px)) ok = interpolate_wrap(src, H, W, (float)py, (float)px, col);
		} else {
			const double px = (lon - F.lon0) / F.step_lon;
			if (!(px < 0 || px >= W || py < 0 || py >= H) && !(px != px)) ok = interpolate(src, H, W, (float)py, (float)px, col);
		}
	}
	float* p = out + ((long long)i * S.out_w + j) * 3;
	if (ok) { p[0] = col[0]; p[1] = col[1]; p[2] = col[2]; }
	else { p[0] = -1.f; p[1] = -1.f; p[2] = -1.f; }
}

template <int MODE, bool WRAP>
void launch_reproject(const op_pano_frame& f, const op_view_spec& s, const op_canvas* c, float* out, hipStream_t st) {
	hipLaunchKernelGGL((k_canvas_reproject<MODE, WRAP>), dim3((s.out_w + 63) / 64, (s.out_h + 3) / 4), dim3(256), 0, st, f, s, c->data, c->h, c->w, out);
}

}	// namespace

extern "C" {

int op_canvas_reproject(op_ctx* ctx, const op_canvas* c, const op_pano_frame* f, const op_view_spec* s, op_canvas** out) {
	if (!ctx || !c || !f || !s || !out) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: bad argument");
	const int rc = reproject_check(f, s);
	if (rc != OP_OK) return rc;
	// the samplers' float bounds are exact up to 2^24 (interpolate_wrap above); the grid's second dimension holds 65535 tiles
	if (c->h > (1 << 24) || c->w > (1 << 24)) OP_FAIL(OP_ERR_UNSUPPORTED, "op_canvas_reproject: a source beyond 2^24 rows or columns");
	if (s->out_h > 65535 || s->out_w > 65535) OP_FAIL(OP_ERR_UNSUPPORTED, "op_canvas_reproject: an output beyond 65535 rows or columns");
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	const size_t n = (size_t)s->out_h * s->out_w * 3;
	CallBlocks own({ctx->stream});
	float* data = nullptr;
	if (own.alloc(&data, sizeof(float) * n) != hipSuccess) OP_FAIL(OP_ERR_HIP, "op_canvas_reproject: allocation failed");
	{ ProfScope ps(ctx, "reproject");
	  if (s->mode == OP_VIEW_PLANET) { if (f->wrap) launch_reproject<OP_VIEW_PLANET, true>(*f, *s, c, data, st); else launch_reproject<OP_VIEW_PLANET, false>(*f, *s, c, data, st); }
	  else { if (f->wrap) launch_reproject<OP_VIEW_RECTILINEAR, true>(*f, *s, c, data, st); else launch_reproject<OP_VIEW_RECTILINEAR, false>(*f, *s, c, data, st); } }
	HIPCHK(hipGetLastError());
	HIPCHK(own.finish());
	resolve_profile(ctx);
	*out = new op_canvas{own.release(data), s->out_h, s->out_w, ctx->device};      // born owning its block, on the last line
	return OP_OK;
}

}	// extern "C"
