// blend.hip -- final warp + blend on the device.
//
// Replaces, for the whole bundle per launch:
//   ConnectedImages::blend            stitch/stitcher_image.cc:116-155 (inverse map per canvas pixel,
//                                     stitch/projection.hh:14-71, Homography::trans homography.hh:53-58)
//   LinearBlender::run                stitch/blender.cc:24-96 (both LAZY_READ branches)
//   MultiBandBlender::run             stitch/multiband.cc:19-151 (+ GaussianBlur::blur<WeightedPixel>,
//                                     feature/gaussian.hh:30-91)
//   interpolate                       lib/imgproc.cc:135-156 (blend_sample.hpp)
//   CylinderProject::project          stitch/warp.cc:25-44 (canvas.hip)
// and keeps on the host, in fp64 with the host libm exactly like the reference, the O(n)
// geometry: calc_inverse_homo / update_proj_range / get_final_resolution
// (stitcher_image.cc:36-114) and the bounds of CylinderProject::project(Shape2D&) (warp.cc:46-67): blend_geom.cc.
// This file: the blend kernels, blend_impl and op_blend*.  The sampler they share with the overlap statistics
// (overlap.hip) is blend_sample.hpp; the canvas handle is canvas.hip; the photometric solvers, photometric_solve.cc.
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
#include "blend_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

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

}	// namespace

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

namespace {

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

}	// extern "C"
