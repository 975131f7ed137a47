// canvas.hip -- the canvas handle (op_canvas_*): copies, the crop to the largest valid rectangle, the byte quantisation;
// and the cylinder pre-warp (op_cyl_warp), whose result is a canvas too.
#include "blend_sample.hpp"

namespace {

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

// ---- CylinderStitcher::perspective_correction's LinearBlender pass (cylstitcher.cc:170-179, blender.cc:24-96) over ONE image,
// the canvas itself: thread per output pixel, 64 x 4 tiles as k_blend_linear.  The ROI is (0, 0)-(W, H) and the target has
// that size, so both branches of run() visit every pixel.  The map is Homography::trans2d(Vec2D(j, i)) (homography.hh:53-76):
// no centre offset and no z < 0 test (space_to_image has both); ImageToAdd::map_coor's bounds (blender.hh:39-44) are tested on
// the doubles, BEFORE the narrowing -- -1e-50 narrows to -0.f, which in_taps would let through -- and what z == 0 makes of
// the coordinates (NaN, +-inf) fails every comparison there or is caught by isNaN() (blender.cc:29), which looks at x.
struct PerspMap { double inv[9]; };
__global__ void __launch_bounds__(256) k_canvas_perspective(PerspMap M, const float* __restrict__ src, int H, int W, float* __restrict__ out,
		int ordered_input, int lazy) {
	const int j = blockIdx.x * 64 + (threadIdx.x & 63);
	const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (i >= H || j >= W) return;
	const double* d = M.inv;
	const double mx = (double)j, my = (double)i;
	const double rx = d[0] * mx + d[1] * my + d[2] * 1.0;
	const double ry = d[3] * mx + d[4] * my + d[5] * 1.0;
	const double rz = d[6] * mx + d[7] * my + d[8] * 1.0;
	const double denom = 1.0 / rz;
	const double ox = rx * denom, oy = ry * denom;
	float s0 = 0.f, s1 = 0.f, s2 = 0.f, wsum = 0.f;
	if (!(ox < 0 || ox >= W || oy < 0 || oy >= H) && !(ox != ox)) {
		const float r = (float)oy, c = (float)ox;
		float col[3];
		if (interpolate(src, H, W, r, c, col) && !(col[0] < 0)) {
			float w = (float)(0.5 - fabs((double)(c / (float)W) - 0.5));
			if (!ordered_input) w = (float)((double)w * (0.5 - fabs((double)(r / (float)H) - 0.5)));
			s0 += col[0] * w; s1 += col[1] * w; s2 += col[2] * w;
			wsum += w;
		}
	}
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
constexpr size_t CROP_LDS_MAX = 150 * 1024;         // of the 160 KiB of a CU; k_crop_lines' static arrays take 4 KiB more
constexpr size_t crop_lds_bytes(int w) { return sizeof(int) * (size_t)(w + (w + CROP_CHUNK - 1) / CROP_CHUNK); }   // hs + cmin
constexpr int crop_max_width() { int w = (int)(CROP_LDS_MAX / sizeof(int)); while (crop_lds_bytes(w) > CROP_LDS_MAX) --w; return w; }
static_assert(crop_max_width() == 37809 && crop_lds_bytes(37809) == CROP_LDS_MAX, "37809 + 591 ints = 150 KiB");
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
// the canvas as bytes: canvas_byte of every float
__global__ void __launch_bounds__(256) k_to_u8(const float* __restrict__ src, long long n, unsigned char* __restrict__ dst) {
	const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
	if (e >= n) return;
	dst[e] = canvas_byte(src[e]);
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
	if (crop_lds_bytes(w) > CROP_LDS_MAX) OP_FAIL(OP_ERR_UNSUPPORTED, "op_canvas_crop: canvas wider than " + std::to_string(crop_max_width()) + " px");
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
	  const size_t lds = crop_lds_bytes(w);
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

int op_canvas_upload(op_ctx* ctx, const float* host_rgb, int h, int w, op_canvas** out) {
	if (!ctx || !host_rgb || !out || h < 1 || w < 1) OP_FAIL(OP_ERR_INVALID, "op_canvas_upload: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	CallBlocks own({ctx->stream});
	float* data = nullptr;
	const size_t bytes = sizeof(float) * 3 * (size_t)h * w;
	if (own.alloc(&data, bytes) != hipSuccess) OP_FAIL(OP_ERR_HIP, "op_canvas_upload: allocation failed");
	HIPCHK(hipMemcpyAsync(data, host_rgb, bytes, hipMemcpyHostToDevice, ctx->stream));
	HIPCHK(own.finish());
	*out = new op_canvas{own.release(data), h, w, ctx->device};      // born owning its block, on the last line
	return OP_OK;
}

int op_canvas_perspective(op_ctx* ctx, const op_config* cfg, const op_canvas* c, const double* inv, op_canvas** out) {
	if (!ctx || !cfg || !c || !inv || !out) OP_FAIL(OP_ERR_INVALID, "op_canvas_perspective: bad argument");
	PerspMap M;
	for (int k = 0; k < 9; ++k) {
		if (!std::isfinite(inv[k])) OP_FAIL(OP_ERR_INVALID, "op_canvas_perspective: inv[" + std::to_string(k) + "] is not finite");
		M.inv[k] = inv[k];
	}
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	const int h = c->h, w = c->w;
	const size_t n = (size_t)h * w * 3;
	CallBlocks own({ctx->stream});
	float* data = nullptr;
	if (own.alloc(&data, sizeof(float) * (n ? n : 1)) != hipSuccess) OP_FAIL(OP_ERR_HIP, "op_canvas_perspective: allocation failed");
	if (n) {
		ProfScope ps(ctx, "perspective");
		hipLaunchKernelGGL(k_canvas_perspective, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, st, M, c->data, h, w, data,
				cfg->ORDERED_INPUT ? 1 : 0, cfg->LAZY_READ ? 1 : 0);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(own.finish());
	resolve_profile(ctx);
	*out = new op_canvas{own.release(data), h, w, ctx->device};      // born owning its block, on the last line
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

}	// extern "C"
