// overlap.hip -- overlap statistics of the blend stage (op_gain_overlap, op_gain_block_overlap, op_vignette_overlap): the
// samples of the linear blender (blend_sample.hpp) on a lattice of the canvas, reduced per pair of views to the sums the
// host solvers (photometric_solve.cc) read.
#include "blend_host.hpp"
#include <algorithm>

namespace {

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

}	// extern "C"
