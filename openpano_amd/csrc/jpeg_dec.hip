// jpeg_dec.hip -- baseline JPEG files decoded on the device into resident views.
//
// Stands in for read_img -> CImg::load -> libjpeg (lib/imgio.cc:67-90, reached from ImageRef::load, stitch/imageref.hh:22-27):
// SOF0, 8 bits, one interleaved scan, YCbCr at 4:4:4 / 4:2:2 / 4:2:0 or grey, any tables (tests/test_gpu_jpeg_craft.py holds it
// to that: tables per component, odd code shapes, every layout of the segments), with or without restart markers.
// Every byte of a view is what libjpeg's default decode gives (ISLOW IDCT, fancy upsampling, JFIF colour conversion).
// The host parses headers only (jpeg_dec_parse.hpp); the entropy-coded data goes up as it is.  Six launches per batch,
// blockIdx.y (or .x where the grid is one workgroup per image) = image:
//   k_jd_scan   one workgroup per image: flags FF 00 and FF D0..D7, a prefix sum (wg_scan_inclusive) compacts the data and yields the table of
//               restart intervals and the number of subsequences of each; any other marker sets the error word;
//   k_jd_sync   one workgroup per image (its restart intervals dealt over up to 64): passes A and B of the self-synchronising Huffman decode (Weissenberger & Schmidt)
//               over subsequences of S bits, rounds separated by barriers, then a prefix sum of the blocks each completes;
//   k_jd_coef   pass C: a lane per subsequence decodes from its true entry state into zeroed [block][64] int16;
//   k_jd_dc     segmented prefix sum of the DC differences per component, reset at interval starts;
//   k_jd_idct   dequantise + jpeg_idct_islow, a thread per block column, then per row, in LDS, to padded sample planes;
//   k_jd_rgb    a thread per output pixel: chroma upsampling and YCbCr -> RGB, bytes written into the view.
// op_views_decode_jpeg_oriented ends in k_jd_rgb_oriented instead when any file of the batch is to be
// turned: the same conversion a 32 x 32 tile of the stored frame at a time, parked in LDS and written in the view's row order.
// The symbol step, the state and the convergence rule are jpeg_dec_core.hpp's, shared with the host model and the serial
// restatement's checks (tests/harness).  All arithmetic is integer: a view is a function of the file alone.
#include "codec_shared.hpp"
#include "jpeg_dec_core.hpp"
#include "jpeg_dec_parse.hpp"
#include "jpeg_exif.hpp"

static_assert(JD_OK == OP_OK && JD_INVALID == OP_ERR_INVALID && JD_UNSUPPORTED == OP_ERR_UNSUPPORTED, "the parser returns the C-ABI's codes");
static_assert(JX_OK == OP_OK && JX_INVALID == OP_ERR_INVALID, "the EXIF reader returns the C-ABI's codes");
static_assert(JD_S444 == OP_JPEG_444 && JD_S420 == OP_JPEG_420 && JD_S422 == OP_JPEG_422 && JD_GREY == OP_JPEG_GREY, "the parser returns the C-ABI's samplings");

namespace {

#define JD_WG 1024         // threads of the one-workgroup-per-image kernels
#define JD_RUN 8           // bytes a thread of k_jd_scan owns per tile

__constant__ unsigned char c_jd_zz_nat[64] = JPEG_ZZ_NAT;

// the interval that holds subsequence s: the largest j with subfirst[j] <= s (subfirst[0] = 0, subfirst[nint] = nsub > s)
__device__ __forceinline__ uint32_t find_interval(const uint32_t* __restrict__ subfirst, uint32_t nint, uint32_t s) {
	uint32_t lo = 0, hi = nint;
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (subfirst[mid] <= s) lo = mid; else hi = mid; }
	return lo;
}

__device__ __forceinline__ void load_tables(const JdImage& I, JdHuff* huff, uint8_t* kinfo, int t, int nt) {
	const uint32_t* src = (const uint32_t*)I.huff; uint32_t* dst = (uint32_t*)huff;
	for (int k = t; k < (int)(8 * sizeof(JdHuff) / 4); k += nt) dst[k] = src[k];
	if (t < 8) kinfo[t] = I.kinfo[t];
}

// ivstart[iv_off + j]: first compacted byte of interval j (nint + 1 entries); subfirst likewise: first subsequence of interval j
__global__ void __launch_bounds__(JD_WG) k_jd_scan(const JdImage* __restrict__ imgs, const unsigned char* __restrict__ in, unsigned char* __restrict__ cmp,
		uint32_t* __restrict__ ivstart, uint32_t* __restrict__ subfirst, JdStatus* __restrict__ status, uint32_t S) {
	__shared__ uint32_t sk[JD_WG], sm[JD_WG];
	__shared__ uint32_t s_err, s_maxl;
	const JdImage& I = imgs[blockIdx.x];
	const int t = threadIdx.x;
	const unsigned char* src = in + I.in_off;
	unsigned char* dst = cmp + I.cmp_off;
	uint32_t* iv = ivstart + I.iv_off; uint32_t* sf = subfirst + I.iv_off;
	const uint32_t n = I.in_len, nint = I.nint;
	if (t == 0) { s_err = 0; s_maxl = 0; }
	__syncthreads();
	uint32_t basek = 0, basem = 0, err = 0;
	for (uint32_t tile = 0; tile < n; tile += JD_WG * JD_RUN) {
		const uint32_t i0 = tile + (uint32_t)t * JD_RUN;
		uint32_t keep = 0, mark = 0;
		unsigned long long bytes = 0;
		uint32_t prev = i0 > 0 && i0 <= n ? src[i0 - 1] : 0;
#pragma unroll
		for (int j = 0; j < JD_RUN; ++j) {
			const uint32_t i = i0 + j;
			if (i >= n) break;
			const uint32_t b = src[i];
			bytes |= (unsigned long long)b << (8 * j);
			if (b == 0xFF) {
				const uint32_t nx = i + 1 < n ? src[i + 1] : 0xFF;
				if (nx == 0) keep |= 1u << j;
				else if ((nx & 0xF8) == 0xD0) mark |= 1u << j;
				else { err |= JD_ERR_MARKER; keep |= 1u << j; }
			} else if (!(prev == 0xFF && (b == 0 || (b & 0xF8) == 0xD0))) keep |= 1u << j;
			prev = b;
		}
		const uint32_t nk = __popc(keep), nm = __popc(mark);
		sk[t] = nk; sm[t] = nm;
		__syncthreads();
		wg_scan_inclusive<JD_WG>(sk, t);
		wg_scan_inclusive<JD_WG>(sm, t);
		uint32_t ok = basek + sk[t] - nk, om = basem + sm[t] - nm;
#pragma unroll
		for (int j = 0; j < JD_RUN; ++j) {
			if (keep >> j & 1) dst[ok++] = (unsigned char)(bytes >> (8 * j));
			if (mark >> j & 1) {
				++om;                                            // the om-th marker ends interval om - 1
				const uint32_t code = src[i0 + j + 1];               // in range: a marker's second byte exists
				if (code != 0xD0 + ((om - 1) & 7)) err |= JD_ERR_MARKER;
				if (om < nint) iv[om] = ok; else err |= JD_ERR_INTERVALS;
			}
		}
		basek += sk[JD_WG - 1]; basem += sm[JD_WG - 1];
		__syncthreads();
	}
	if (basem + 1 != nint) err |= JD_ERR_INTERVALS;
	if (err) atomicOr(&s_err, err);
	if (t == 0) { iv[0] = 0; iv[nint] = basek; }
	__syncthreads();
	if (s_err) { if (t == 0) { status[blockIdx.x].err = s_err; status[blockIdx.x].ncompact = basek; } return; }
	// subsequences per interval, their exclusive prefix sum, the longest interval
	uint32_t base = 0, maxl = 0;
	for (uint32_t tile = 0; tile < nint; tile += JD_WG) {
		const uint32_t j = tile + t;
		const uint32_t ns = j < nint ? jd_nsub(8u * (iv[j + 1] - iv[j]), S) : 0;
		maxl = max(maxl, ns);
		sk[t] = ns;
		__syncthreads();
		wg_scan_inclusive<JD_WG>(sk, t);
		if (j < nint) sf[j] = base + sk[t] - ns;
		base += sk[JD_WG - 1];
		__syncthreads();
	}
	atomicMax(&s_maxl, maxl);
	__syncthreads();
	if (t == 0) {
		sf[nint] = base;
		JdStatus& st = status[blockIdx.x];
		st.err = base > I.sub_cap ? (uint32_t)JD_ERR_CAP : 0u; st.ncompact = basek; st.nsub = base; st.maxl = s_maxl;
	}
}

// passes A and B.  Restart intervals are independent, so an image's intervals are dealt over gridDim.x workgroups (one
// when the scan is unbroken); blockIdx.y = image.  state0 / state1: the two exit-state arrays the rounds alternate between,
// the final states end in state0.  pex: exclusive prefix sum, over the workgroup's subsequences, of the blocks each completes
// (pass C takes differences inside one interval only).
__global__ void __launch_bounds__(JD_WG) k_jd_sync(const JdImage* __restrict__ imgs, const unsigned char* __restrict__ cmp, const uint32_t* __restrict__ ivstart,
		const uint32_t* __restrict__ subfirst, unsigned long long* state0, unsigned long long* state1, uint32_t* __restrict__ pex,
		JdStatus* __restrict__ status, uint32_t S) {
	__shared__ JdHuff huff[8];
	__shared__ uint8_t kinfo[8];
	__shared__ uint32_t sc[JD_WG];
	JdStatus& st = status[blockIdx.y];
	if (st.err) return;
	const JdImage& I = imgs[blockIdx.y];
	const uint32_t nint = I.nint;
	const uint32_t ja = (uint32_t)((unsigned long long)nint * blockIdx.x / gridDim.x), jb = (uint32_t)((unsigned long long)nint * (blockIdx.x + 1) / gridDim.x);
	if (ja == jb) return;
	const int t = threadIdx.x;
	load_tables(I, huff, kinfo, t, JD_WG);
	__syncthreads();
	const unsigned char* d = cmp + I.cmp_off;
	const uint32_t* iv = ivstart + I.iv_off; const uint32_t* sf = subfirst + I.iv_off;
	const uint32_t s0 = sf[ja], s1 = sf[jb], maxl = st.maxl;      // this workgroup's subsequences: whole intervals
	const int bpm = (int)I.bpm;
	unsigned long long* A = state0 + I.sub_off; unsigned long long* B = state1 + I.sub_off;      // a round reads A and writes B
	int rounds = 0;
	for (uint32_t r = 0; r < (maxl > 1 ? maxl : 1u); ++r) {
		int any = 0;
		for (uint32_t s = s0 + t; s < s1; s += JD_WG) {
			const unsigned long long own = r ? A[s] : 0ull, pred = r && s > s0 ? A[s - 1] : 0ull;
			unsigned long long out;
			if (r && !(pred & 1)) out = own & ~1ull;
			else {
				const uint32_t j = find_interval(sf, nint, s), l = s - sf[j];
				const uint32_t b0 = 8u * iv[j], e = 8u * iv[j + 1];
				const uint32_t sb = b0 + l * S, se = e - sb > S ? sb + S : e;
				out = jd_sub_round(d, sb, se, e, l == 0, (int)r, pred, own, huff, kinfo, bpm);
			}
			B[s] = out;
			any |= (int)(out & 1);
		}
		unsigned long long* x = A; A = B; B = x;
		if (r) ++rounds;
		if (!__syncthreads_or(any)) break;
	}
	// the final states are in A; pass C reads state0
	if (A != state0 + I.sub_off) {
		for (uint32_t s = s0 + t; s < s1; s += JD_WG) B[s] = A[s];
		__syncthreads();
	}
	const unsigned long long* F = state0 + I.sub_off;
	uint32_t base = 0;
	for (uint32_t tile = s0; tile < s1; tile += JD_WG) {
		const uint32_t s = tile + t;
		const uint32_t c = s < s1 ? jd_count(F[s]) : 0;
		sc[t] = c;
		__syncthreads();
		wg_scan_inclusive<JD_WG>(sc, t);
		if (s < s1) pex[I.sub_off + s] = base + sc[t] - c;
		base += sc[JD_WG - 1];
		__syncthreads();
	}
	if (t == 0 && rounds) atomicMax(&st.rounds, (uint32_t)rounds);
}

// pass C
__global__ void __launch_bounds__(256) k_jd_coef(const JdImage* __restrict__ imgs, const unsigned char* __restrict__ cmp, const uint32_t* __restrict__ ivstart,
		const uint32_t* __restrict__ subfirst, const unsigned long long* __restrict__ state0,
		const uint32_t* __restrict__ pex, short* __restrict__ coef, JdStatus* __restrict__ status, uint32_t S) {
	__shared__ JdHuff huff[8];
	__shared__ uint8_t kinfo[8];
	__shared__ uint8_t zz_nat[64];
	JdStatus& st = status[blockIdx.y];
	if (st.err || blockIdx.x * 256u >= st.nsub) return;
	const JdImage& I = imgs[blockIdx.y];
	const int t = threadIdx.x;
	load_tables(I, huff, kinfo, t, 256);
	if (t < 64) zz_nat[t] = c_jd_zz_nat[t];
	__syncthreads();
	const uint32_t s = blockIdx.x * 256u + t;
	if (s >= st.nsub) return;
	const unsigned char* d = cmp + I.cmp_off;
	const uint32_t* iv = ivstart + I.iv_off; const uint32_t* sf = subfirst + I.iv_off;
	const unsigned long long* A = state0 + I.sub_off;
	const uint32_t* px = pex + I.sub_off;
	const int bpm = (int)I.bpm;
	const uint32_t j = find_interval(sf, I.nint, s), l = s - sf[j];
	const uint32_t b0 = 8u * iv[j], e = 8u * iv[j + 1];
	const uint32_t sb = b0 + l * S, se = e - sb > S ? sb + S : e;
	const bool last = s + 1 == sf[j + 1];
	const uint32_t m1 = (j + 1) * I.ri < I.nmcu ? (j + 1) * I.ri : I.nmcu;
	const uint32_t limit = m1 * I.bpm;                                   // one past the interval's last block
	uint32_t blk = j * I.ri * I.bpm + (px[s] - px[sf[j]]);               // the block in progress on entry
	JdCur c;
	if (l == 0) { c.pos = b0; c.k = 0; c.zz = 0; } else c = jd_unpack(A[s - 1]);
	c.n = 0;
	short* out = coef + I.coef_off;
	uint32_t err = 0;
	while (c.pos < se) {
		if (blk >= limit) { if (!jd_tail_is_padding(last, c, e)) err |= JD_ERR_COUNT; break; }      // behind the last block: the bits that pad the interval to a byte
		int idx = 0, val = 0;
		const uint32_t fl = jd_step(d, e, huff, kinfo, bpm, c, idx, val);
		err |= fl & 0xFFu;
		if (fl & JD_COEF) out[(unsigned long long)blk * 64 + zz_nat[idx & 63]] = (short)val;
		if (fl & JD_BLOCK_DONE) ++blk;
	}
	if (last && (blk != limit || c.zz)) err |= JD_ERR_COUNT;
	if (err) atomicOr(&st.err, err);
}

// DC differences -> DC values: blockIdx.x = component; the component's blocks in scan order, a new segment at every interval start
__global__ void __launch_bounds__(JD_WG) k_jd_dc(const JdImage* __restrict__ imgs, short* __restrict__ coef, const JdStatus* __restrict__ status) {
	__shared__ int sv[JD_WG];
	__shared__ int sfl[JD_WG];
	__shared__ int s_carry;
	const JdImage& I = imgs[blockIdx.y];
	const int c = blockIdx.x, t = threadIdx.x;
	if (status[blockIdx.y].err || c >= I.ncomp) return;
	const uint32_t ny = I.ncomp == 1 ? 1u : (uint32_t)(I.hs * I.vs);
	const uint32_t bc = c ? 1u : ny, koff = c ? ny + c - 1 : 0u, total = I.nmcu * bc;
	short* co = coef + I.coef_off;
	int carry = 0;
	for (uint32_t tile = 0; tile < total; tile += JD_WG) {
		const uint32_t el = tile + t;
		const uint32_t m = el / bc, sub = el - m * bc;
		const unsigned long long at = ((unsigned long long)m * I.bpm + koff + sub) * 64;
		int v = 0, f = 0;
		if (el < total) { v = co[at]; f = sub == 0 && m % I.ri == 0; }
		sv[t] = v; sfl[t] = f;
		__syncthreads();
		for (int off = 1; off < JD_WG; off <<= 1) {
			int pv = 0, pf = 0;
			if (t >= off) { pv = sv[t - off]; pf = sfl[t - off]; }
			__syncthreads();
			if (t >= off) { if (!sfl[t]) sv[t] += pv; sfl[t] |= pf; }
			__syncthreads();
		}
		int r = sv[t];
		if (!sfl[t]) r += carry;
		if (el < total) co[at] = (short)r;
		if (t == JD_WG - 1) s_carry = r;
		__syncthreads();
		carry = s_carry;
		__syncthreads();
	}
}

// 32 blocks per workgroup
__global__ void __launch_bounds__(256) k_jd_idct(const JdImage* __restrict__ imgs, const short* __restrict__ coef, unsigned char* __restrict__ planes,
		const JdStatus* __restrict__ status) {
	__shared__ int ws[32 * 72];      // rows of 9 ints: both passes free of bank conflicts
	const JdImage& I = imgs[blockIdx.y];
	if (status[blockIdx.y].err || blockIdx.x * 32u >= I.nblocks) return;
	const int t = threadIdx.x, lb = t >> 3, cr = t & 7;
	const uint32_t b = blockIdx.x * 32u + lb;
	const bool live = b < I.nblocks;
	const uint32_t m = live ? b / I.bpm : 0, k = live ? b - m * I.bpm : 0;
	const int comp = jd_kinfo_comp(I.kinfo[k]);
	if (live) {
		const short* in = coef + I.coef_off + (unsigned long long)b * 64 + cr;
		const uint8_t* q = I.q[comp] + cr;
		int o[8];
		jd_idct_pass<11>(in[0] * q[0], in[8] * q[8], in[16] * q[16], in[24] * q[24], in[32] * q[32], in[40] * q[40], in[48] * q[48], in[56] * q[56], o);
#pragma unroll
		for (int r = 0; r < 8; ++r) ws[lb * 72 + r * 9 + cr] = o[r];
	}
	__syncthreads();
	if (!live) return;
	const int* w = ws + lb * 72 + cr * 9;
	int o[8];
	jd_idct_pass<18>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
	const int hsc = comp ? 1 : I.hs, sub = comp ? 0 : (int)k;
	const int mx = (int)(m % (uint32_t)I.mcuw), my = (int)(m / (uint32_t)I.mcuw);
	const int bx = mx * hsc + (sub % hsc), by = my * (comp ? 1 : I.vs) + (sub / hsc);
	unsigned long long v = 0;
#pragma unroll
	for (int x = 0; x < 8; ++x) v |= (unsigned long long)jd_clamp255(o[x] + 128) << (8 * x);
	unsigned char* p = planes + I.plane_off[comp] + ((long long)by * 8 + cr) * I.plane_w[comp] + bx * 8;
	*(unsigned long long*)p = v;      // planes start at multiples of 256 bytes and their pitch is a multiple of 8
}

__global__ void __launch_bounds__(256) k_jd_rgb(const JdImage* __restrict__ imgs, const unsigned char* __restrict__ planes, unsigned char* __restrict__ views,
		const JdStatus* __restrict__ status) {
	const JdImage& I = imgs[blockIdx.y];
	if (status[blockIdx.y].err) return;
	const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
	if (p >= (long long)I.h * I.w) return;
	const int y = (int)(p / I.w), x = (int)(p - (long long)y * I.w);
	const int Y = planes[I.plane_off[0] + (long long)y * I.plane_w[0] + x];
	unsigned char* o = views + I.out_off + 3 * p;
	if (I.ncomp == 1) { o[0] = o[1] = o[2] = (unsigned char)Y; return; }
	const int cw = (I.w + I.hs - 1) / I.hs, ch = (I.h + I.vs - 1) / I.vs;
	const int Cb = jd_chroma(planes + I.plane_off[1], I.plane_w[1], cw, ch, I.hs, I.vs, y, x);
	const int Cr = jd_chroma(planes + I.plane_off[2], I.plane_w[2], cw, ch, I.hs, I.vs, y, x);
	uint8_t rgb[3];
	jd_ycc_rgb(Y, Cb, Cr, rgb);
	o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

// ---- the last stage of op_views_decode_jpeg_oriented: k_jd_rgb's conversion, the view turned by the EXIF orientation ----
#define JD_OT 32                     // the tile of the stored frame a workgroup of k_jd_rgb_oriented owns: JD_OT x JD_OT pixels
#define JD_OT_PITCH (JD_OT + 1)      // dwords of a tile row in LDS: the odd pitch spreads a tile column over all 32 banks

// what k_jd_rgb_oriented knows about a file beyond JdImage, which stays as the other kernels read it
struct JdOrient { int32_t orient, oh, ow, tiles_x; };      // orient 1..8; oh x ow: the view; tiles_x: tiles across the stored frame

// An orientation is three bits: the view is the stored frame mirrored in x (2, 3, 7, 8), mirrored in y (3, 4, 6, 7), then
// transposed (5..8).  A workgroup converts its tile in source order (lanes along a stored row: coalesced reads of the sample
// planes), parks a pixel per dword in LDS and writes the tile in the view's row order (lanes along a row of the view: every
// row of the tile is one run of 3 * JD_OT bytes).  Both LDS passes are dword accesses of 32-lane groups: along a tile row
// the banks are consecutive, along a tile column they step by JD_OT_PITCH = 33 = 1 (mod 32), so neither serialises.
__global__ void __launch_bounds__(256) k_jd_rgb_oriented(const JdImage* __restrict__ imgs, const JdOrient* __restrict__ orient,
		const unsigned char* __restrict__ planes, unsigned char* __restrict__ views, const JdStatus* __restrict__ status) {
	__shared__ uint32_t tile[JD_OT * JD_OT_PITCH];
	const JdImage& I = imgs[blockIdx.y];
	const JdOrient O = orient[blockIdx.y];
	if (status[blockIdx.y].err) return;
	const int ty = (int)(blockIdx.x / (unsigned)O.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)O.tiles_x);
	const int y0 = ty * JD_OT, x0 = tx * JD_OT;
	if (y0 >= I.h) return;                                   // uniform over the workgroup: no barrier is skipped by a part of it
	const int r = threadIdx.x >> 5, c = threadIdx.x & 31;
	const int cw = (I.w + I.hs - 1) / I.hs, ch = (I.h + I.vs - 1) / I.vs;
	const int x = x0 + c;
#pragma unroll
	for (int k = 0; k < JD_OT; k += 8) {
		const int y = y0 + r + k;
		if (y >= I.h || x >= I.w) continue;
		const int Y = planes[I.plane_off[0] + (long long)y * I.plane_w[0] + x];
		uint32_t px;
		if (I.ncomp == 1) px = (uint32_t)Y * 0x010101u;
		else {
			const int Cb = jd_chroma(planes + I.plane_off[1], I.plane_w[1], cw, ch, I.hs, I.vs, y, x);
			const int Cr = jd_chroma(planes + I.plane_off[2], I.plane_w[2], cw, ch, I.hs, I.vs, y, x);
			uint8_t rgb[3];
			jd_ycc_rgb(Y, Cb, Cr, rgb);
			px = (uint32_t)rgb[0] | (uint32_t)rgb[1] << 8 | (uint32_t)rgb[2] << 16;
		}
		tile[(r + k) * JD_OT_PITCH + c] = px;
	}
	__syncthreads();
	const int o = O.orient - 1;
	const bool tr = o >= 4, fx = o == 1 || o == 2 || o == 6 || o == 7, fy = o == 2 || o == 3 || o == 5 || o == 6;
	unsigned char* out = views + I.out_off;
#pragma unroll
	for (int k = 0; k < JD_OT; k += 8) {
		// (r + k, c): row and column of the tile as the view sees it; lanes run along the view's row, ascending
		const int along = tr ? (fy ? JD_OT - 1 - c : c) : (fx ? JD_OT - 1 - c : c);
		const int ly = tr ? along : r + k, lx = tr ? r + k : along;
		const int sy = y0 + ly, sx = x0 + lx;
		if (sy >= I.h || sx >= I.w) continue;
		const int my = fy ? I.h - 1 - sy : sy, mx = fx ? I.w - 1 - sx : sx;
		const int oy = tr ? mx : my, ox = tr ? my : mx;
		const uint32_t px = tile[ly * JD_OT_PITCH + lx];
		unsigned char* q = out + 3 * ((long long)oy * O.ow + ox);
		q[0] = (unsigned char)px; q[1] = (unsigned char)(px >> 8); q[2] = (unsigned char)(px >> 16);
	}
}

std::string err_text(uint32_t e) {
	std::string s;
	auto add = [&](const char* m) { if (!s.empty()) s += "; "; s += m; };
	if (e & JD_ERR_MARKER) add("a marker other than RSTn in the entropy-coded data, or RSTn out of order");
	if (e & JD_ERR_INTERVALS) add("the number of restart intervals is not the frame's");
	if (e & JD_ERR_CODE) add("bits that are no Huffman code");
	if (e & JD_ERR_INDEX) add("a run past coefficient 63");
	if (e & JD_ERR_CAT) add("a coefficient category out of range");
	if (e & JD_ERR_END) add("a symbol runs past the end of its restart interval");
	if (e & JD_ERR_COUNT) add("an interval does not hold the frame's number of blocks");
	if (e & JD_ERR_CAP) add("internal: subsequence capacity");
	return s;
}

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the body of op_views_decode_jpeg (oriented = false: `orientation` is not read) and of op_views_decode_jpeg_oriented; fn names the entry in messages
int decode_views(op_ctx* ctx, const unsigned char* const* files, const int64_t* sizes, int n, bool oriented, const int* orientation,
		const std::string& fn, op_views** out) {
	if (!ctx || !files || !sizes || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, fn + ": bad argument");
	*out = nullptr;
	if (oriented && orientation)
		for (int i = 0; i < n; ++i)
			if (orientation[i] < 0 || orientation[i] > 8)
				OP_FAIL(OP_ERR_INVALID, fn + ": file " + std::to_string(i) + ": orientation " + std::to_string(orientation[i]) + " is neither 0 (the file's EXIF) nor 1..8");
	// ---- headers: every refusal happens here, before anything is allocated or launched
	std::vector<JdImage> imgs((size_t)n);
	std::vector<int64_t> scan_begin((size_t)n);
	std::vector<JdOrient> orient;      // read only when some file is to be turned: otherwise the launches are op_views_decode_jpeg's
	bool turned = false;
	if (oriented) orient.resize((size_t)n);
	{
		HostScope hs(ctx, "jpegdec parse (host)");
		for (int i = 0; i < n; ++i) {
			if (!files[i] || sizes[i] < 0) OP_FAIL(OP_ERR_INVALID, fn + ": file " + std::to_string(i) + ": NULL data or negative size");
			JdHeader H;
			const int r = jd_parse(files[i], sizes[i], H);
			if (r != JD_OK) OP_FAIL(r, fn + ": file " + std::to_string(i) + ": " + H.why);
			jd_describe(H, imgs[i]);
			scan_begin[i] = H.scan_begin;
			if (oriented) {
				int o = orientation ? orientation[i] : 0;
				if (o == 0) { JxExif X; jx_exif(files[i], sizes[i], X); o = X.orientation; }
				turned |= o != 1;
				orient[i] = JdOrient{o, o >= 5 ? H.w : H.h, o >= 5 ? H.h : H.w, (H.w + JD_OT - 1) / JD_OT};
			}
		}
	}
	const uint32_t S = ctx->jpeg_subseq_bits ? (uint32_t)ctx->jpeg_subseq_bits : (uint32_t)JD_S_DEFAULT;
	size_t in_total = 0, cmp_total = 0, iv_total = 0, sub_total = 0, coef_total = 0, plane_total = 0, out_total = 0;
	uint32_t max_sub = 0, max_blocks = 0, max_int = 0; long long max_px = 0, max_tiles = 0;
	for (int i = 0; i < n; ++i) {
		JdImage& I = imgs[i];
		I.in_off = in_total; in_total += up((size_t)I.in_len + 1, 16);
		I.cmp_off = cmp_total; cmp_total += up((size_t)I.in_len + JD_PAD, 16);
		I.iv_off = (uint32_t)iv_total; iv_total += (size_t)I.nint + 1;
		I.sub_cap = (uint32_t)(((unsigned long long)I.in_len * 8 + S - 1) / S) + I.nint;
		I.sub_off = (uint32_t)sub_total; sub_total += I.sub_cap;
		I.coef_off = coef_total; coef_total += (size_t)I.nblocks * 64;
		for (int c = 0; c < I.ncomp; ++c) { I.plane_off[c] = plane_total; plane_total += up((size_t)I.plane_w[c] * I.plane_h[c], 256); }
		I.out_off = out_total; out_total += up((size_t)3 * I.h * I.w, 256);
		max_int = std::max(max_int, I.nint); max_sub = std::max(max_sub, I.sub_cap); max_blocks = std::max(max_blocks, I.nblocks);
		max_px = std::max(max_px, (long long)I.h * I.w);
		max_tiles = std::max(max_tiles, (long long)((I.h + JD_OT - 1) / JD_OT) * ((I.w + JD_OT - 1) / JD_OT));
	}
	// k_jd_sync: about JD_WG subsequences per workgroup, never more workgroups than intervals
	const uint32_t sync_wgs = std::max(1u, std::min(std::min(max_int, 64u), (max_sub + JD_WG - 1) / JD_WG));
	if (iv_total >= (1ull << 31) || sub_total >= (1ull << 31)) OP_FAIL(OP_ERR_UNSUPPORTED, fn + ": the batch holds more than 2^31 restart intervals or subsequences: split it");
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	CallBlocks own({st});
	JdImage* d_imgs = nullptr; unsigned char *d_in = nullptr, *d_cmp = nullptr, *d_planes = nullptr; char* block = nullptr;
	uint32_t *d_iv = nullptr, *d_sf = nullptr, *d_pex = nullptr; unsigned long long *d_s0 = nullptr, *d_s1 = nullptr;
	short* d_coef = nullptr; JdStatus* d_status = nullptr; JdOrient* d_orient = nullptr;
	HIPCHK(own.alloc(&d_imgs, sizeof(JdImage) * (size_t)n));
	HIPCHK(own.alloc(&d_in, in_total));
	HIPCHK(own.alloc(&d_cmp, cmp_total));
	HIPCHK(own.alloc(&d_iv, sizeof(uint32_t) * iv_total));
	HIPCHK(own.alloc(&d_sf, sizeof(uint32_t) * iv_total));
	HIPCHK(own.alloc(&d_s0, sizeof(unsigned long long) * sub_total));
	HIPCHK(own.alloc(&d_s1, sizeof(unsigned long long) * sub_total));
	HIPCHK(own.alloc(&d_pex, sizeof(uint32_t) * sub_total));
	HIPCHK(own.alloc(&d_coef, sizeof(short) * coef_total));
	HIPCHK(own.alloc(&d_planes, plane_total));
	HIPCHK(own.alloc(&d_status, sizeof(JdStatus) * (size_t)n));
	HIPCHK(own.alloc(&block, out_total));
	if (turned) HIPCHK(own.alloc(&d_orient, sizeof(JdOrient) * (size_t)n));
	{ ProfScope ps(ctx, "jpegdec H2D");
	  HIPCHK(hipMemcpyAsync(d_imgs, imgs.data(), sizeof(JdImage) * (size_t)n, hipMemcpyHostToDevice, st));
	  if (turned) HIPCHK(hipMemcpyAsync(d_orient, orient.data(), sizeof(JdOrient) * (size_t)n, hipMemcpyHostToDevice, st));
	  for (int i = 0; i < n; ++i)
		if (imgs[i].in_len) HIPCHK(hipMemcpyAsync(d_in + imgs[i].in_off, files[i] + scan_begin[i], imgs[i].in_len, hipMemcpyHostToDevice, st));
	  HIPCHK(hipMemsetAsync(d_status, 0, sizeof(JdStatus) * (size_t)n, st));
	  HIPCHK(hipMemsetAsync(d_coef, 0, sizeof(short) * coef_total, st)); }
	{ ProfScope ps(ctx, "jpegdec scan");
	  hipLaunchKernelGGL(k_jd_scan, dim3(n), dim3(JD_WG), 0, st, d_imgs, d_in, d_cmp, d_iv, d_sf, d_status, S);
	  HIPCHK(hipGetLastError()); }
	{ ProfScope ps(ctx, "jpegdec sync");
	  hipLaunchKernelGGL(k_jd_sync, dim3(sync_wgs, n), dim3(JD_WG), 0, st, d_imgs, d_cmp, d_iv, d_sf, d_s0, d_s1, d_pex, d_status, S);
	  HIPCHK(hipGetLastError()); }
	{ ProfScope ps(ctx, "jpegdec coef");
	  hipLaunchKernelGGL(k_jd_coef, dim3((max_sub + 255) / 256, n), dim3(256), 0, st, d_imgs, d_cmp, d_iv, d_sf, d_s0, d_pex, d_coef, d_status, S);
	  HIPCHK(hipGetLastError()); }
	{ ProfScope ps(ctx, "jpegdec dc");
	  hipLaunchKernelGGL(k_jd_dc, dim3(3, n), dim3(JD_WG), 0, st, d_imgs, d_coef, d_status);
	  HIPCHK(hipGetLastError()); }
	{ ProfScope ps(ctx, "jpegdec idct");
	  hipLaunchKernelGGL(k_jd_idct, dim3((max_blocks + 31) / 32, n), dim3(256), 0, st, d_imgs, d_coef, d_planes, d_status);
	  HIPCHK(hipGetLastError()); }
	if (!turned) {
		ProfScope ps(ctx, "jpegdec rgb");
		hipLaunchKernelGGL(k_jd_rgb, dim3((unsigned)((max_px + 255) / 256), n), dim3(256), 0, st, d_imgs, d_planes, (unsigned char*)block, d_status);
		HIPCHK(hipGetLastError());
	} else {      // the whole batch, identity included as a case
		ProfScope ps(ctx, "jpegdec rgb oriented (k_jd_rgb_oriented)");
		hipLaunchKernelGGL(k_jd_rgb_oriented, dim3((unsigned)max_tiles, n), dim3(256), 0, st, d_imgs, d_orient, d_planes, (unsigned char*)block, d_status);
		HIPCHK(hipGetLastError());
	}
	std::vector<JdStatus> status((size_t)n);
	HIPCHK(hipMemcpyAsync(status.data(), d_status, sizeof(JdStatus) * (size_t)n, hipMemcpyDeviceToHost, st));
	HIPCHK(own.finish());      // the caller's files are free again
	resolve_profile(ctx);
	int rounds = 0;
	for (int i = 0; i < n; ++i) {
		if (status[i].err) OP_FAIL(OP_ERR_INVALID, fn + ": file " + std::to_string(i) + ": " + err_text(status[i].err));
		rounds = std::max(rounds, (int)status[i].rounds);
	}
	ctx->jpeg_last_rounds = rounds;
	op_views* v = new op_views;
	v->ctx = ctx; v->block = own.release(block);
	v->imgs.resize((size_t)n);
	for (int i = 0; i < n; ++i) {
		const bool swap = turned && orient[i].orient >= 5;
		v->imgs[i] = op_image{block + imgs[i].out_off, swap ? imgs[i].w : imgs[i].h, swap ? imgs[i].h : imgs[i].w, 1, OP_U8};
	}
	*out = v;
	return OP_OK;
}


}	// namespace

extern "C" {

int op_jpeg_probe(const unsigned char* file, int64_t size, int* h, int* w, int* sampling) {
	if (!file || size < 0) OP_FAIL(OP_ERR_INVALID, "op_jpeg_probe: bad argument");
	JdHeader H;
	const int r = jd_parse(file, size, H);
	if (r != JD_OK) OP_FAIL(r, "op_jpeg_probe: " + H.why);
	if (h) *h = H.h;
	if (w) *w = H.w;
	if (sampling) *sampling = H.sampling;
	return OP_OK;
}

int op_debug_set_jpeg_subseq_bits(op_ctx* ctx, int bits) {
	if (!ctx || bits < 0 || bits % 32 || bits > JD_S_MAX) OP_FAIL(OP_ERR_INVALID, "op_debug_set_jpeg_subseq_bits: bad argument (0, or a multiple of 32 up to 65536)");
	ctx->jpeg_subseq_bits = bits;
	return OP_OK;
}

int op_debug_jpeg_last_rounds(op_ctx* ctx) {
	if (!ctx) OP_FAIL(OP_ERR_INVALID, "op_debug_jpeg_last_rounds: NULL context");
	return ctx->jpeg_last_rounds;
}

int op_jpeg_exif(const unsigned char* file, int64_t size, int* orientation, int* focal35) {
	if (!file || size < 0) OP_FAIL(OP_ERR_INVALID, "op_jpeg_exif: bad argument");
	JxExif X;
	if (jx_exif(file, size, X) != JX_OK) OP_FAIL(OP_ERR_INVALID, "op_jpeg_exif: no SOI: not a JPEG file");
	if (orientation) *orientation = X.orientation;
	if (focal35) *focal35 = X.focal35;
	return OP_OK;
}

int op_views_decode_jpeg(op_ctx* ctx, const unsigned char* const* files, const int64_t* sizes, int n, op_views** out) {
	return decode_views(ctx, files, sizes, n, false, nullptr, "op_views_decode_jpeg", out);
}

int op_views_decode_jpeg_oriented(op_ctx* ctx, const unsigned char* const* files, const int64_t* sizes, int n, const int* orientation, op_views** out) {
	return decode_views(ctx, files, sizes, n, true, orientation, "op_views_decode_jpeg_oriented", out);
}

int op_views_copy(op_ctx* ctx, const op_views* v, int i, void* host) {
	if (!ctx || !v || !host || i < 0 || i >= (int)v->imgs.size()) OP_FAIL(OP_ERR_INVALID, "op_views_copy: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	const op_image& im = v->imgs[i];
	const size_t bytes = (im.dtype == OP_U8 ? 1 : sizeof(float)) * 3 * (size_t)im.h * im.w;
	HIPCHK(hipMemcpyAsync(host, im.data, bytes, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return OP_OK;
}

}	// extern "C"
